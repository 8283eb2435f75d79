// Composition of caller-built supervisions with the normalization acceptor of a denominator graph: what
// [K] AddWeightToSupervisionFst (chain-supervision.cc) does to every supervision Kaldi writes into an eg, and what the
// end-to-end egs do with --normalization-fst-scale.  Host code only: it runs once per utterance, when a supervision is made.
//
// The normalization acceptor N of a graph ([K] DenominatorGraph::GetNormalizationFst, epsilon-removed): the states of
// den.fst plus a start q0; every arc h -> h' (pdf p, probability w) at cost -log w; for every h with pi(h) > 0 and every
// arc h -> h' an arc q0 -> h' with label p at cost -log pi(h) - log w; every state final at cost 0.  pi are the handle's
// initial probabilities, w its arc probabilities: the float32 values the denominator kernels use.  An arc of probability 0
// is on no path and is left out.  The leaky-HMM coefficient does not enter.
//
// The output of a sequence is the product of its acceptor with N, trimmed, in a fixed order (tests/den_compose_reference.py
// restates it): breadth-first from (s_0, q0); states in increasing new id, their supervision arcs in input order, for each
// the matching arcs of N in the order the handle keeps the graph's arcs (q0: source state ascending, then its arcs); a new
// state gets the next id when first reached; trimming keeps the relative order.  Parallel arcs of N stay parallel arcs:
// nothing is determinised or minimised, so a non-deterministic den.fst is summed over, not maximised.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>

#include "chain_internal.h"

struct tc_den_compose_result {
  int32_t S = 0;
  std::vector<int32_t> seq_state_begin, start, arc_begin, ilabel, nextstate, status;
  std::vector<float> arc_weight, final_weight;
  std::vector<int64_t> info;  // [S][4]: states, arcs of the input; states, arcs of the output
};

namespace {

// N's arcs by (source, label): sources 0 .. H - 1 are the graph's states, source H is q0.  Inside one (source, label) the
// arcs keep the order stated above.
struct NormArc {
  int32_t dst;
  double cost;
};
struct NormFst {
  int32_t H = 0;
  std::vector<int64_t> state_begin;  // [H + 2] into key_pdf / key_begin's rows
  std::vector<int32_t> key_pdf;      // per (source, label) group, ascending inside a source
  std::vector<int64_t> key_begin;    // [groups + 1] into arcs
  std::vector<NormArc> arcs;

  // the arcs of `src` that carry `pdf`: [*lo, *hi)
  void match(int32_t src, int32_t pdf, int64_t *lo, int64_t *hi) const {
    const int32_t *b = key_pdf.data() + state_begin[src], *e = key_pdf.data() + state_begin[src + 1];
    const int32_t *it = std::lower_bound(b, e, pdf);
    if (it == e || *it != pdf) {
      *lo = *hi = 0;
      return;
    }
    const int64_t k = it - key_pdf.data();
    *lo = key_begin[k];
    *hi = key_begin[k + 1];
  }
};

void build_norm(const tc_den_graph *g, NormFst *n) {
  struct Raw {
    int32_t src, pdf, dst;
    double cost;
  };
  const int32_t H = g->H;
  std::vector<Raw> raw;
  raw.reserve((size_t)g->A * 2);
  for (int64_t a = 0; a < g->A; ++a) {
    if (!(g->arc_prob[a] > 0.f)) continue;
    raw.push_back(Raw{g->arc_src[a], g->arc_pdf[a], g->arc_dst[a], -std::log((double)g->arc_prob[a])});
  }
  // (the graph's arcs are state-major -- tc_den_graph_create refuses anything else -- so this is h ascending, then its arcs)
  for (int64_t a = 0; a < g->A; ++a) {
    const float pi = g->initial_probs[g->arc_src[a]];
    if (!(g->arc_prob[a] > 0.f) || !(pi > 0.f)) continue;
    raw.push_back(Raw{H, g->arc_pdf[a], g->arc_dst[a], -std::log((double)pi) - std::log((double)g->arc_prob[a])});
  }
  std::stable_sort(raw.begin(), raw.end(), [](const Raw &x, const Raw &y) { return x.src != y.src ? x.src < y.src : x.pdf < y.pdf; });
  n->H = H;
  n->state_begin.assign((size_t)H + 2, 0);
  n->arcs.reserve(raw.size());
  size_t i = 0;
  for (int32_t s = 0; s <= H; ++s) {
    n->state_begin[s] = (int64_t)n->key_pdf.size();
    while (i < raw.size() && raw[i].src == s) {
      if (n->key_pdf.size() == (size_t)n->state_begin[s] || n->key_pdf.back() != raw[i].pdf) {
        n->key_pdf.push_back(raw[i].pdf);
        n->key_begin.push_back((int64_t)n->arcs.size());
      }
      n->arcs.push_back(NormArc{raw[i].dst, raw[i].cost});
      ++i;
    }
  }
  n->state_begin[H + 1] = (int64_t)n->key_pdf.size();
  n->key_begin.push_back((int64_t)n->arcs.size());
}

struct SeqOut {
  std::vector<int32_t> arc_begin, ilabel, nextstate;  // arc_begin: n + 1 entries from 0
  std::vector<float> arc_weight, final_weight;
};

// One sequence: n states, arcs [ab[i], ab[i + 1]) of the concatenated arrays for local state i.  Returns the status.
int compose_one(const NormFst &N, int32_t n, int32_t start, const int32_t *ab, const int32_t *il, const float *aw,
                const int32_t *nx, const float *fin, double scale, int64_t max_states, SeqOut *out) {
  const int64_t width = (int64_t)N.H + 1;
  std::unordered_map<int64_t, int32_t> id_of;
  std::vector<int32_t> sup_of, den_of;  // per product state
  std::vector<int64_t> p_begin(1, 0);
  std::vector<int32_t> p_label, p_next;
  std::vector<float> p_cost;
  id_of.emplace((int64_t)start * width + N.H, 0);
  sup_of.push_back(start);
  den_of.push_back(N.H);
  for (size_t q = 0; q < sup_of.size(); ++q) {
    const int32_t s = sup_of[q], h = den_of[q];
    for (int32_t a = ab[s]; a < ab[s + 1]; ++a) {
      int64_t lo, hi;
      N.match(h, il[a] - 1, &lo, &hi);
      for (int64_t k = lo; k < hi; ++k) {
        const int64_t key = (int64_t)nx[a] * width + N.arcs[k].dst;
        auto it = id_of.find(key);
        int32_t to;
        if (it == id_of.end()) {
          if ((int64_t)sup_of.size() >= max_states) return 2;
          to = (int32_t)sup_of.size();
          id_of.emplace(key, to);
          sup_of.push_back(nx[a]);
          den_of.push_back(N.arcs[k].dst);
        } else {
          to = it->second;
        }
        p_label.push_back(il[a]);
        p_next.push_back(to);
        p_cost.push_back((float)((double)aw[a] + scale * N.arcs[k].cost));
      }
    }
    p_begin.push_back((int64_t)p_label.size());
  }
  // trim: every state is reachable by construction; keep those from which a final state is
  const int32_t np = (int32_t)sup_of.size();
  std::vector<int64_t> in_begin((size_t)np + 1, 0);
  for (int32_t to : p_next) ++in_begin[to + 1];
  for (int32_t q = 0; q < np; ++q) in_begin[q + 1] += in_begin[q];
  std::vector<int32_t> in_src(p_next.size());
  {
    std::vector<int64_t> fill(in_begin.begin(), in_begin.end() - 1);
    for (int32_t q = 0; q < np; ++q)
      for (int64_t a = p_begin[q]; a < p_begin[q + 1]; ++a) in_src[fill[p_next[a]]++] = q;
  }
  std::vector<char> keep(np, 0);
  std::vector<int32_t> stack;
  for (int32_t q = 0; q < np; ++q)
    if (!std::isinf(fin[sup_of[q]])) keep[q] = 1, stack.push_back(q);
  while (!stack.empty()) {
    const int32_t q = stack.back();
    stack.pop_back();
    for (int64_t a = in_begin[q]; a < in_begin[q + 1]; ++a)
      if (!keep[in_src[a]]) keep[in_src[a]] = 1, stack.push_back(in_src[a]);
  }
  if (!keep[0]) return 1;
  std::vector<int32_t> new_id(np, -1);
  int32_t kept = 0;
  for (int32_t q = 0; q < np; ++q)
    if (keep[q]) new_id[q] = kept++;
  out->arc_begin.assign(1, 0);
  for (int32_t q = 0; q < np; ++q) {
    if (!keep[q]) continue;
    for (int64_t a = p_begin[q]; a < p_begin[q + 1]; ++a) {
      if (!keep[p_next[a]]) continue;
      out->ilabel.push_back(p_label[a]);
      out->nextstate.push_back(new_id[p_next[a]]);
      out->arc_weight.push_back(p_cost[a]);
    }
    if (out->ilabel.size() > (size_t)std::numeric_limits<int32_t>::max()) return 2;
    out->arc_begin.push_back((int32_t)out->ilabel.size());
    out->final_weight.push_back(fin[sup_of[q]]);
  }
  return 0;
}

}  // namespace

extern "C" {

int tc_den_graph_arcs(const tc_den_graph *g, int32_t *src, int32_t *dst, int32_t *pdf, float *prob) {
  if (!g) return TC_ERR_INVALID_ARGUMENT;
  const size_t A = (size_t)g->A;
  if (src) memcpy(src, g->arc_src.data(), A * sizeof(int32_t));
  if (dst) memcpy(dst, g->arc_dst.data(), A * sizeof(int32_t));
  if (pdf) memcpy(pdf, g->arc_pdf.data(), A * sizeof(int32_t));
  if (prob) memcpy(prob, g->arc_prob.data(), A * sizeof(float));
  return TC_OK;
}

int tc_den_compose(tc_den_compose_result **out, const tc_den_graph *g, int32_t S, int32_t label_dim, int e2e,
                   const int32_t *seq_state_begin, const int32_t *start, const int32_t *arc_begin, const int32_t *ilabel,
                   const float *arc_weight, const int32_t *nextstate, const float *final_weight, float scale,
                   int64_t max_states) {
  if (!out) return TC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!g || S <= 0 || label_dim <= 0 || !seq_state_begin || !arc_begin || !final_weight || (e2e && !start))
    return TC_ERR_INVALID_ARGUMENT;
  if (!(scale >= 0.f) || std::isinf(scale) || max_states < 1) return TC_ERR_INVALID_ARGUMENT;
  // the input, validated as tc_supervision_create_ragged / tc_supervision_create_e2e validate it, before anything is indexed
  if (seq_state_begin[0] != 0) return TC_ERR_BAD_FST;
  for (int32_t s = 0; s < S; ++s)
    if (seq_state_begin[s + 1] <= seq_state_begin[s]) return TC_ERR_BAD_FST;  // (a sequence has a start state)
  const int32_t num_states = seq_state_begin[S];
  if (arc_begin[0] != 0) return TC_ERR_BAD_FST;
  for (int32_t i = 0; i < num_states; ++i)
    if (arc_begin[i + 1] < arc_begin[i]) return TC_ERR_BAD_FST;
  const int32_t num_arcs = arc_begin[num_states];
  if (num_arcs > 0 && (!ilabel || !arc_weight || !nextstate)) return TC_ERR_INVALID_ARGUMENT;
  const float ninf = -std::numeric_limits<float>::infinity();
  for (int32_t s = 0; s < S; ++s) {
    const int32_t sb = seq_state_begin[s], n = seq_state_begin[s + 1] - sb;
    if (e2e && (start[s] < 0 || start[s] >= n)) return TC_ERR_BAD_FST;
    for (int32_t i = 0; i < n; ++i)
      if (std::isnan(final_weight[sb + i]) || final_weight[sb + i] == ninf) return TC_ERR_BAD_FST;
    for (int32_t a = arc_begin[sb]; a < arc_begin[sb + n]; ++a) {
      if (ilabel[a] < 1 || ilabel[a] > label_dim) return TC_ERR_BAD_FST;  // 0: epsilon
      if (nextstate[a] < 0 || nextstate[a] >= n) return TC_ERR_BAD_FST;
      if (std::isnan(arc_weight[a]) || arc_weight[a] == ninf) return TC_ERR_BAD_FST;
    }
  }

  NormFst N;  // (built per call from the handle's immutable arrays: the handle is only read, from any number of threads)
  build_norm(g, &N);
  tc_den_compose_result *r = new tc_den_compose_result;
  r->S = S;
  r->seq_state_begin.assign(1, 0);
  r->arc_begin.assign(1, 0);
  r->start.assign(S, 0);
  r->status.assign(S, 0);
  r->info.assign((size_t)S * 4, 0);
  for (int32_t s = 0; s < S; ++s) {
    const int32_t sb = seq_state_begin[s], n = seq_state_begin[s + 1] - sb;
    SeqOut o;
    const int st = compose_one(N, n, e2e ? start[s] : 0, arc_begin + sb, ilabel, arc_weight, nextstate, final_weight + sb,
                               (double)scale, max_states, &o);
    r->status[s] = st;
    r->info[4 * s + 0] = n;
    r->info[4 * s + 1] = arc_begin[sb + n] - arc_begin[sb];
    if (st == 0) {
      const int64_t ns = (int64_t)o.final_weight.size(), na = (int64_t)o.ilabel.size();
      if ((int64_t)r->final_weight.size() + ns > std::numeric_limits<int32_t>::max() ||
          (int64_t)r->ilabel.size() + na > std::numeric_limits<int32_t>::max()) {
        r->status[s] = 2;  // (the concatenated arrays are indexed by int32, as the create calls' are)
      } else {
        const int32_t abase = (int32_t)r->ilabel.size();
        for (size_t i = 1; i < o.arc_begin.size(); ++i) r->arc_begin.push_back(abase + o.arc_begin[i]);
        r->ilabel.insert(r->ilabel.end(), o.ilabel.begin(), o.ilabel.end());
        r->nextstate.insert(r->nextstate.end(), o.nextstate.begin(), o.nextstate.end());
        r->arc_weight.insert(r->arc_weight.end(), o.arc_weight.begin(), o.arc_weight.end());
        r->final_weight.insert(r->final_weight.end(), o.final_weight.begin(), o.final_weight.end());
        r->info[4 * s + 2] = ns;
        r->info[4 * s + 3] = na;
      }
    }
    r->seq_state_begin.push_back((int32_t)r->final_weight.size());
  }
  *out = r;
  return TC_OK;
}

int tc_den_compose_sizes(const tc_den_compose_result *r, int64_t *out3) {
  if (!r || !out3) return TC_ERR_INVALID_ARGUMENT;
  out3[0] = r->S;
  out3[1] = (int64_t)r->final_weight.size();
  out3[2] = (int64_t)r->ilabel.size();
  return TC_OK;
}

int tc_den_compose_info(const tc_den_compose_result *r, int32_t *status, int64_t *info4) {
  if (!r) return TC_ERR_INVALID_ARGUMENT;
  if (status) memcpy(status, r->status.data(), r->status.size() * sizeof(int32_t));
  if (info4) memcpy(info4, r->info.data(), r->info.size() * sizeof(int64_t));
  return TC_OK;
}

int tc_den_compose_copy(const tc_den_compose_result *r, int32_t *seq_state_begin, int32_t *start, int32_t *arc_begin,
                        int32_t *ilabel, float *arc_weight, int32_t *nextstate, float *final_weight) {
  if (!r) return TC_ERR_INVALID_ARGUMENT;
  auto put = [](void *dst, const void *src, size_t bytes) {
    if (dst && bytes) memcpy(dst, src, bytes);
  };
  put(seq_state_begin, r->seq_state_begin.data(), r->seq_state_begin.size() * 4);
  put(start, r->start.data(), r->start.size() * 4);
  put(arc_begin, r->arc_begin.data(), r->arc_begin.size() * 4);
  put(ilabel, r->ilabel.data(), r->ilabel.size() * 4);
  put(arc_weight, r->arc_weight.data(), r->arc_weight.size() * 4);
  put(nextstate, r->nextstate.data(), r->nextstate.size() * 4);
  put(final_weight, r->final_weight.data(), r->final_weight.size() * 4);
  return TC_OK;
}

void tc_den_compose_free(tc_den_compose_result *r) { delete r; }

}  // extern "C"
