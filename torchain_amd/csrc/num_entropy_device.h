// The arithmetic the entropy kernels of REGULAR supervisions share (num_entropy_regular_kernels.hip, the level-windowed one, and
// num_entropy_wide_kernels.hip, the wide-level one): the posterior mean of a state, E[log W] over the final states, and the
// store of a gradient element.  log alpha, log beta, log Z and the occupations are num_device.h's.  One statement of each, so
// that on a handle both kernels serve they give the same bits.
#pragma once

#include <math.h>

#include <type_traits>

#include "half_io.h"

namespace tc {

template <typename El>
__device__ __forceinline__ void entr_store(void *g, int64_t i, float v) {
  if constexpr (std::is_same<El, float>::value)
    reinterpret_cast<float *>(g)[i] = v;
  else
    reinterpret_cast<uint16_t *>(g)[i] = Elem<El>::round(v);
}

// The posterior mean of val(a) = mean(other state of a) + r_a over one state's arc list, `acc` being the list's log-sum
// (num_state_log_sum over the same list): other(a) gives the other state's pair (log weight, mean).
template <class ArcAt, class Score, class Other>
__device__ __forceinline__ double entr_state_mean(int i0, int i1, double acc, ArcAt arc_at, Score score, Other other) {
  if (!(acc > -INFINITY)) return 0.0;  // no path through the state: its mean is never weighted
  double num = 0.0, den = 0.0;
  for (int i = i0; i < i1; ++i) {
    const int a = arc_at(i);
    const double r = (double)score(a);
    const double2 o = other(a);
    const float sh = __expf((float)(r + o.x - acc));
    if (sh > 0.f) {  // (a share of 0 may stand before an infinite cost or a state without a path)
      num += (double)sh * (o.y + r);
      den += (double)sh;
    }
  }
  return num / den;
}

// E[log W] of a sequence: the final states f0 .. f1 - 1 share log Z = `tot` (num_total over the same states) by the float32 exp
// of (log alpha + final log-weight - log Z); pair(st) gives a final state's (log alpha, Abar).  One lane, in state order.
template <class Pair>
__device__ __forceinline__ double entr_final_mean(int f0, int f1, const float *final_logw, double tot, Pair pair) {
  double num = 0.0, den = 0.0;
  if (tot > -INFINITY)
    for (int st = f0; st < f1; ++st) {
      const double fl = (double)final_logw[st];
      if (fl == -INFINITY) continue;
      const double2 l = pair(st);
      const float sh = __expf((float)(l.x + fl - tot));
      if (sh > 0.f) {
        num += (double)sh * (l.y + fl);
        den += (double)sh;
      }
    }
  return num / den;
}

}  // namespace tc
