#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "chain_internal.h"
#include "torchain_hip.h"
// tc_supervision_create_ragged, and tc_supervision_create on each sequence alone, over corrupted copies of valid arrays
// (ASan/UBSan build, host only): both entries build a sequence's tables in the same function of csrc/supervision.cpp.
// input file: int32 S, P, num_states, num_arcs; float weight; then frames[S], seq_state_begin[S+1], arc_begin[ns+1], ilabel[na],
// next[na] (int32), arc_weight[na], final[ns] (float)
namespace tc {
// (den_graph.cpp's, which is not part of this program)
thread_local int g_last_hip_error = 0;
bool debug_flag(DebugFlag) { return false; }
}
int main(int argc, char **argv) {
  FILE *f = fopen(argv[1], "rb");
  int32_t hdr[4];
  float weight;
  if (!f || fread(hdr, 4, 4, f) != 4 || fread(&weight, 4, 1, f) != 1) return 2;
  const int S = hdr[0], P = hdr[1], ns = hdr[2], na = hdr[3];
  std::vector<int32_t> fr(S), sb(S + 1), ab(ns + 1), il(na), nx(na);
  std::vector<float> w(na), fin(ns);
  if (fread(fr.data(), 4, S, f) != (size_t)S || fread(sb.data(), 4, S + 1, f) != (size_t)S + 1 ||
      fread(ab.data(), 4, ns + 1, f) != (size_t)ns + 1 || fread(il.data(), 4, na, f) != (size_t)na ||
      fread(nx.data(), 4, na, f) != (size_t)na || fread(w.data(), 4, na, f) != (size_t)na || fread(fin.data(), 4, ns, f) != (size_t)ns)
    return 2;
  fclose(f);
  int ok = 0, bad = 0;
  auto run = [&](std::vector<int32_t> &frames, std::vector<int32_t> &begin, std::vector<int32_t> &a, std::vector<int32_t> &l,
                 std::vector<int32_t> &n, std::vector<float> &ww, std::vector<float> &ff, int p) {
    tc_supervision *h = nullptr;
    const int rc = tc_supervision_create_ragged(&h, weight, S, frames.data(), p, begin.data(), a.data(), l.data(), ww.data(), n.data(),
                                                ff.data());
    if (rc == 0) {
      ++ok;
      int64_t stats[12];
      std::vector<int32_t> got(S);
      if (tc_supervision_stats(h, stats) != 0 || tc_supervision_frames(h, got.data()) != 0 || !tc_supervision_is_ragged(h)) abort();
      tc_supervision_free(h);
    } else {
      ++bad;
    }
  };
  run(fr, sb, ab, il, nx, w, fin, P);
  if (ok != 1) return 3;
  srand(3);
  for (int i = 0; i < 4000; ++i) {
    std::vector<int32_t> frames = fr, begin = sb, a = ab, l = il, n = nx;
    std::vector<float> ww = w, ff = fin;
    int p = P;
    const int what = rand() % 9, k = 1 + rand() % 3;
    for (int j = 0; j < k; ++j) switch (what) {
      // (the arrays hold arc_begin[num_states] arcs and seq_state_begin[S] states: the caller's contract)
      case 0: { const size_t ix = rand() % a.size(); a[ix] += (rand() % 7) - 3; if (ix + 1 == a.size() && a[ix] > na) a[ix] = na; } break;
      case 1: l[rand() % l.size()] = (rand() % (2 * P + 4)) - 2; break;
      case 2: n[rand() % n.size()] = (rand() % (ns + 6)) - 3; break;
      case 3: ww[rand() % ww.size()] = (rand() % 3 == 0) ? __builtin_inff() : (float)(rand() % 100) - 50.f; break;
      case 4: ff[rand() % ff.size()] = (rand() % 2) ? 0.f : __builtin_inff(); break;
      case 5: frames[rand() % S] += (rand() % 5) - 2; break;
      case 6: { const size_t ix = rand() % begin.size(); begin[ix] += (rand() % 5) - 2; if (begin[ix] > ns) begin[ix] = ns; if (ix + 1 == begin.size() && begin[ix] > ns) begin[ix] = ns; } break;
      case 7: { const int x = rand() % n.size(), y = rand() % n.size(); std::swap(n[x], n[y]); } break;
      case 8: p = P + (rand() % 5) - 2; break;
    }
    if (begin.back() > ns) begin.back() = ns;
    run(frames, begin, a, l, n, ww, ff, p);
  }
  printf("create_ragged: ok %d refused %d\n", ok, bad);
  // the uniform entry on every sequence alone: the same builder behind the split
  ok = bad = 0;
  for (int s = 0; s < S; ++s) {
    const int n0 = sb[s], n1 = sb[s + 1], a0 = ab[n0];
    std::vector<int32_t> a(ab.begin() + n0, ab.begin() + n1 + 1);
    for (auto &x : a) x -= a0;
    tc_supervision *h = nullptr;
    const int rc = tc_supervision_create(&h, weight, 1, fr[s], P, n1 - n0, a.data(), il.data() + a0, w.data() + a0, nx.data() + a0,
                                         fin.data() + n0);
    if (rc == 0) { ++ok; tc_supervision_free(h); } else ++bad;
  }
  printf("create on each sequence alone: ok %d refused %d\n", ok, bad);
  return bad ? 4 : 0;
}
