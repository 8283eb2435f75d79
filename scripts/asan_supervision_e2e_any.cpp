#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "chain_internal.h"
#include "torchain_hip.h"
// tc_supervision_create_e2e_any and tc_supervision_e2e_stats (csrc/supervision_e2e.cpp) under ASan/UBSan, host only: sequences
// at the resident kernel's limits, one past each, at the new LDS rule and one past it, uniform and ragged, beside the two
// older entries on the same arrays; then 3000 corrupted copies of a small valid batch.
namespace tc {
// (den_graph.cpp's, which is not part of this program)
thread_local int g_last_hip_error = 0;
static bool g_force = false;
bool debug_flag(DebugFlag f) { return f == kDbgForceNumE2eLarge && g_force; }
}  // namespace tc

namespace {
struct Batch {
  std::vector<int32_t> sb{0}, start, ab{0}, il, nx;
  std::vector<float> w, fin;
  // a ring of `states` with extra arcs up to `arcs`, over the pdfs 0 .. pdfs - 1
  void add(int states, int arcs, int pdfs) {
    std::vector<std::vector<int>> out(states);
    for (int i = 0; i < states; ++i) out[i].push_back(i);
    for (int k = states; k < arcs; ++k) out[k % states].push_back(k);
    for (int i = 0; i < states; ++i) {
      for (int k : out[i]) {
        il.push_back(k % pdfs + 1);
        nx.push_back(k < states ? (k + 1) % states : (int)(((int64_t)k * 7 + 3) % states));
        w.push_back(0.1f);
      }
      ab.push_back((int32_t)il.size());
      fin.push_back(i == 0 ? 0.f : INFINITY);
    }
    sb.push_back(sb.back() + states);
    start.push_back(0);
  }
  int S() const { return (int)start.size(); }
};

int create(const Batch &b, int T, const int32_t *frames, int P, int entry, int64_t *stats) {
  tc_supervision *h = nullptr;
  const int S = b.S();
  int rc;
  if (entry == 0)
    rc = tc_supervision_create_e2e_any(&h, 1.f, S, T, frames, P, b.sb.data(), b.start.data(), b.ab.data(), b.il.data(), b.w.data(),
                                       b.nx.data(), b.fin.data());
  else if (frames)
    rc = tc_supervision_create_e2e_ragged(&h, 1.f, S, frames, P, b.sb.data(), b.start.data(), b.ab.data(), b.il.data(), b.w.data(),
                                          b.nx.data(), b.fin.data());
  else
    rc = tc_supervision_create_e2e(&h, 1.f, S, T, P, b.sb.data(), b.start.data(), b.ab.data(), b.il.data(), b.w.data(), b.nx.data(),
                                   b.fin.data());
  if (rc == 0) {
    if (!h || !tc_supervision_is_e2e(h)) abort();
    int64_t st[8];
    std::vector<int32_t> got(S);
    if (tc_supervision_e2e_stats(h, st) != 0 || tc_supervision_frames(h, got.data()) != 0) abort();
    if (tc_supervision_is_ragged(h) != (frames ? 1 : 0)) abort();
    for (int s = 0; s < S; ++s)
      if (got[s] != (frames ? frames[s] : T)) abort();
    int64_t regular[12];
    if (tc_supervision_stats(h, regular) != TC_ERR_INVALID_ARGUMENT) abort();
    if (stats)
      for (int i = 0; i < 8; ++i) stats[i] = st[i];
    tc_supervision_free(h);
  } else if (h) {
    abort();
  }
  return rc;
}

void expect(const char *what, int got, int want) {
  printf("%-58s %d\n", what, got);
  if (got != want) {
    printf("  expected %d\n", want);
    exit(3);
  }
}
}  // namespace

int main() {
  const int P = 7700;
  const int32_t lens[2] = {4, 10};
  struct Size { const char *name; int states, arcs, pdfs, any_rc, old_rc, route; };
  const Size sizes[] = {
      {"at the resident limits", 2048, 8192, 1024, 0, 0, 0},
      {"one state past", 2049, 8192, 1024, 0, TC_ERR_UNSUPPORTED, 1},
      {"one arc past", 2048, 8193, 1024, 0, TC_ERR_UNSUPPORTED, 1},
      {"one pdf past", 2048, 8192, 1025, 0, TC_ERR_UNSUPPORTED, 1},
      {"at the LDS rule (8192 states, 7680 pdfs)", 8192, 9000, 7680, 0, TC_ERR_UNSUPPORTED, 1},
      {"one pdf past the LDS rule", 8192, 9000, 7681, TC_ERR_UNSUPPORTED, TC_ERR_UNSUPPORTED, 1},
      {"one state past the LDS rule", 8193, 9000, 7680, TC_ERR_UNSUPPORTED, TC_ERR_UNSUPPORTED, 1},
      {"at the LDS rule (10108 states, 4 pdfs)", 10108, 12000, 4, 0, TC_ERR_UNSUPPORTED, 1},
      {"10109 states", 10109, 12000, 4, TC_ERR_UNSUPPORTED, TC_ERR_UNSUPPORTED, 1},
      {"200000 arcs on 300 states", 300, 200000, 50, 0, TC_ERR_UNSUPPORTED, 1},
  };
  for (const Size &z : sizes) {
    Batch b;
    b.add(3, 3, 1);
    b.add(z.states, z.arcs, z.pdfs);
    printf("%s\n", z.name);
    int64_t st[8] = {0};
    expect("  create_e2e_any, uniform", create(b, 10, nullptr, P, 0, st), z.any_rc);
    if (z.any_rc == 0) {
      if (st[0] != 2 || st[1] != z.states || st[2] != z.arcs || st[3] != z.pdfs || st[7] != z.route) abort();
      if (st[5] + 2048 > tc::kLdsLimitBytes || st[4] != st[5] + 4 * (int64_t)z.arcs) abort();
      tc::g_force = true;
      int64_t forced[8];
      expect("  create_e2e_any under the force switch", create(b, 10, nullptr, P, 0, forced), 0);
      tc::g_force = false;
      if (forced[7] != 1 || forced[6] < st[6] || (z.route == 0 && forced[6] == st[6])) abort();
    }
    expect("  create_e2e_any, ragged", create(b, 0, lens, P, 0, nullptr), z.any_rc);
    expect("  create_e2e", create(b, 10, nullptr, P, 1, nullptr), z.old_rc);
    expect("  create_e2e_ragged", create(b, 0, lens, P, 1, nullptr), z.old_rc);
    // a malformed sequence beside it: the structure is reported, not the size
    Batch bad = b;
    bad.il[1] = 0;
    expect("  an epsilon arc beside it", create(bad, 10, nullptr, P, 0, nullptr), TC_ERR_BAD_FST);
    bad = b;
    bad.nx.back() = z.states;
    expect("  a next state out of range in it", create(bad, 10, nullptr, P, 0, nullptr), TC_ERR_BAD_FST);
  }
  {
    // the rule is per sequence: the largest state count and the largest pdf count in two sequences, each at the rule
    Batch b;
    b.add(10108, 12000, 4);
    b.add(8192, 16000, 7680);
    int64_t st[8];
    expect("10108 states / 4 pdfs beside 8192 states / 7680 pdfs", create(b, 6, nullptr, P, 0, st), 0);
    if (st[1] != 10108 || st[3] != 7680 || st[5] != 16 * 8192 + 4 * 7680 || st[5] + 2048 > tc::kLdsLimitBytes || st[7] != 1) abort();
  }
  {
    Batch b;
    b.add(2049, 8192, 1024);
    const int T = (int)(((int64_t)4 << 30) / (8 * 2049)) + 1;
    expect("history above 4 GiB", create(b, T, nullptr, P, 0, nullptr), TC_ERR_UNSUPPORTED);
    const int32_t zero[1] = {0};
    expect("a length of 0 frames", create(b, 0, zero, P, 0, nullptr), TC_ERR_INVALID_ARGUMENT);
    expect("no frames", create(b, 0, nullptr, P, 0, nullptr), TC_ERR_INVALID_ARGUMENT);
    expect("null out", tc_supervision_create_e2e_any(nullptr, 1.f, 1, 5, nullptr, P, b.sb.data(), b.start.data(), b.ab.data(),
                                                     b.il.data(), b.w.data(), b.nx.data(), b.fin.data()), TC_ERR_INVALID_ARGUMENT);
    tc_supervision *h = nullptr;
    expect("null arcs", tc_supervision_create_e2e_any(&h, 1.f, 1, 5, nullptr, P, b.sb.data(), b.start.data(), b.ab.data(), nullptr,
                                                      b.w.data(), b.nx.data(), b.fin.data()), TC_ERR_INVALID_ARGUMENT);
    int64_t st[8];
    expect("stats of a null handle", tc_supervision_e2e_stats(nullptr, st), TC_ERR_INVALID_ARGUMENT);
  }
  // corrupted copies of a small valid batch, through the new entry (uniform and ragged in turn)
  Batch good;
  good.add(5, 12, 4);
  good.add(9, 30, 7);
  const int ns = good.sb.back(), na = good.ab.back();
  int ok = 0, refused = 0;
  srand(5);
  for (int i = 0; i < 3000; ++i) {
    Batch b = good;
    int p = 12;
    int32_t fr[2] = {6, 3};
    const int what = rand() % 9, k = 1 + rand() % 3;
    for (int j = 0; j < k; ++j) switch (what) {
      // (the arrays hold arc_begin[num_states] arcs and seq_state_begin[S] states: the caller's contract)
      case 0: { const size_t ix = rand() % b.ab.size(); b.ab[ix] += (rand() % 7) - 3; if (b.ab[ix] > na) b.ab[ix] = na; } break;
      case 1: b.il[rand() % na] = (rand() % (2 * p + 4)) - 2; break;
      case 2: b.nx[rand() % na] = (rand() % (ns + 6)) - 3; break;
      case 3: b.w[rand() % na] = (rand() % 3 == 0) ? (rand() % 2 ? INFINITY : -INFINITY) : (rand() % 5 == 0 ? NAN : (float)(rand() % 100) - 50.f); break;
      case 4: b.fin[rand() % ns] = (rand() % 3 == 0) ? NAN : (rand() % 2 ? 0.f : INFINITY); break;
      case 5: fr[rand() % 2] += (rand() % 9) - 4; break;
      case 6: { const size_t ix = rand() % b.sb.size(); b.sb[ix] += (rand() % 5) - 2; if (b.sb[ix] > ns) b.sb[ix] = ns; } break;
      case 7: b.start[rand() % 2] = (rand() % 14) - 2; break;
      case 8: p = 12 + (rand() % 14) - 8; break;
    }
    if (b.sb.back() > ns) b.sb.back() = ns;
    if (b.sb.back() < 0) b.sb.back() = 0;
    // (arc_begin is read up to its entry seq_state_begin[S], and the arc arrays up to arc_begin's value there)
    (create(b, 6, i % 2 ? fr : nullptr, p, 0, nullptr) == 0 ? ok : refused)++;
  }
  printf("corrupted copies: ok %d refused %d\n", ok, refused);
  return ok > 0 && refused > 0 ? 0 : 4;
}
