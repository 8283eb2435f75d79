#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "chain_internal.h"
#include "torchain_hip.h"
// tc_den_compose over corrupted copies of a valid batch (ASan/UBSan build, host only), regular and end-to-end form; every
// accepted output goes through the create call of its form (csrc/supervision.cpp, csrc/supervision_e2e.cpp).
// input file: int32 H, A, P, S, num_states, num_arcs; then the graph: src[A], dst[A], ilabel[A] (int32), weight[A], final[H]
// (float); then the batch: frames[S], seq_state_begin[S+1], arc_begin[ns+1], ilabel[na], next[na] (int32), arc_weight[na],
// final[ns] (float)
int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  int32_t hdr[6];
  if (!f || fread(hdr, 4, 6, f) != 6) return 2;
  const int H = hdr[0], A = hdr[1], P = hdr[2], S = hdr[3], ns = hdr[4], na = hdr[5];
  std::vector<int32_t> gs(A), gd(A), gl(A), fr(S), sb(S + 1), ab(ns + 1), il(na), nx(na);
  std::vector<float> gw(A), gf(H), w(na), fin(ns);
  auto rd = [&](void *p, size_t n) { return fread(p, 4, n, f) == n; };
  if (!rd(gs.data(), A) || !rd(gd.data(), A) || !rd(gl.data(), A) || !rd(gw.data(), A) || !rd(gf.data(), H) || !rd(fr.data(), S) ||
      !rd(sb.data(), S + 1) || !rd(ab.data(), ns + 1) || !rd(il.data(), na) || !rd(nx.data(), na) || !rd(w.data(), na) ||
      !rd(fin.data(), ns))
    return 2;
  fclose(f);
  tc_den_graph *g = nullptr;
  if (tc_den_graph_create(&g, H, A, gs.data(), gd.data(), gl.data(), gw.data(), gf.data(), 0, P) != 0) return 3;
  // the graph as the handle keeps it: read again at the end (the composition only reads it)
  auto snapshot = [&]() {
    std::vector<int32_t> a(3 * (size_t)A);
    std::vector<float> b((size_t)A + H);
    if (tc_den_graph_arcs(g, a.data(), a.data() + A, a.data() + 2 * (size_t)A, b.data()) != 0 || tc_den_graph_initial_probs(g, b.data() + A) != 0)
      abort();
    std::vector<char> out(a.size() * 4 + b.size() * 4);
    memcpy(out.data(), a.data(), a.size() * 4);
    memcpy(out.data() + a.size() * 4, b.data(), b.size() * 4);
    return out;
  };
  const std::vector<char> before = snapshot();
  int ok = 0, bad = 0, empty = 0, large = 0, created = 0;
  auto run = [&](int e2e, std::vector<int32_t> &begin, std::vector<int32_t> &start, std::vector<int32_t> &a, std::vector<int32_t> &l,
                 std::vector<int32_t> &n, std::vector<float> &ww, std::vector<float> &ff, int p, float scale, int64_t max_states) {
    tc_den_compose_result *r = nullptr;
    const int rc = tc_den_compose(&r, g, S, p, e2e, begin.data(), start.data(), a.data(), l.data(), ww.data(), n.data(), ff.data(),
                                  scale, max_states);
    if (rc != 0) {
      if (r) abort();
      ++bad;
      return;
    }
    ++ok;
    int64_t sz[3];
    if (tc_den_compose_sizes(r, sz) != 0 || sz[0] != S) abort();
    std::vector<int32_t> st(S), osb(S + 1), ost(S), oab(sz[1] + 1), oil(sz[2]), onx(sz[2]);
    std::vector<int64_t> info(4 * (size_t)S);
    std::vector<float> ow(sz[2]), ofin(sz[1]);
    if (tc_den_compose_info(r, st.data(), info.data()) != 0 ||
        tc_den_compose_copy(r, osb.data(), ost.data(), oab.data(), oil.data(), ow.data(), onx.data(), ofin.data()) != 0)
      abort();
    tc_den_compose_free(r);
    bool all = true;
    for (int s = 0; s < S; ++s) {
      empty += st[s] == 1;
      large += st[s] == 2;
      all = all && st[s] == 0;
      if ((st[s] == 0) != (osb[s + 1] > osb[s]) || info[4 * s + 2] != osb[s + 1] - osb[s]) abort();
    }
    if (osb[S] != sz[1] || oab[sz[1]] != sz[2]) abort();
    if (!all) return;
    tc_supervision *h = nullptr;
    const int rc2 = e2e ? tc_supervision_create_e2e(&h, 1.f, S, 12, p, osb.data(), ost.data(), oab.data(), oil.data(), ow.data(),
                                                   onx.data(), ofin.data())
                        : tc_supervision_create_ragged(&h, 1.f, S, fr.data(), p, osb.data(), oab.data(), oil.data(), ow.data(),
                                                      onx.data(), ofin.data());
    // (a corrupted copy that still composes may no longer be time-unfolded: the regular create call may refuse it, not crash)
    if (rc2 == 0) { ++created; tc_supervision_free(h); }
  };
  std::vector<int32_t> start0(S, 0);
  for (int e2e = 0; e2e < 2; ++e2e) {
    ok = bad = empty = large = created = 0;
    run(e2e, sb, start0, ab, il, nx, w, fin, P, 1.f, 200000);
    if (ok != 1 || created != 1) return 4;
    srand(3 + e2e);
    for (int i = 0; i < 4000; ++i) {
      std::vector<int32_t> begin = sb, start = start0, a = ab, l = il, n = nx;
      std::vector<float> ww = w, ff = fin;
      int p = P;
      float scale = (float)(rand() % 3) * 0.5f;
      int64_t max_states = 200000;
      const int what = rand() % 10, k = 1 + rand() % 3;
      for (int j = 0; j < k; ++j) switch (what) {
        // (the arrays hold arc_begin[num_states] arcs and seq_state_begin[S] states: the caller's contract)
        case 0: { const size_t ix = rand() % a.size(); a[ix] += (rand() % 7) - 3; if (ix + 1 == a.size() && a[ix] > na) a[ix] = na; } break;
        case 1: l[rand() % l.size()] = (rand() % (2 * P + 4)) - 2; break;
        case 2: n[rand() % n.size()] = (rand() % (ns + 6)) - 3; break;
        case 3: ww[rand() % ww.size()] = (rand() % 3 == 0) ? (rand() % 2 ? __builtin_inff() : __builtin_nanf("")) : (float)(rand() % 100) - 50.f; break;
        case 4: ff[rand() % ff.size()] = (rand() % 3 == 0) ? -__builtin_inff() : ((rand() % 2) ? 0.f : __builtin_inff()); break;
        case 5: start[rand() % S] = (rand() % 12) - 2; break;
        case 6: { const size_t ix = rand() % begin.size(); begin[ix] += (rand() % 5) - 2; if (begin[ix] > ns) begin[ix] = ns; } break;
        case 7: { const int x = rand() % n.size(), y = rand() % n.size(); std::swap(n[x], n[y]); } break;
        case 8: p = P + (rand() % 5) - 2; break;
        case 9: max_states = 1 + rand() % 40; scale = (rand() % 4 == 0) ? -1.f : scale; break;
      }
      if (begin.back() > ns) begin.back() = ns;
      if (a.back() > na) a.back() = na;
      run(e2e, begin, start, a, l, n, ww, ff, p, scale, max_states);
    }
    printf("%s: composed %d refused %d; sequences empty %d, over max_states %d; handles created %d\n", e2e ? "end-to-end" : "regular",
           ok, bad, empty, large, created);
  }
  if (snapshot() != before) return 5;
  tc_den_graph_free(g);
  return 0;
}
