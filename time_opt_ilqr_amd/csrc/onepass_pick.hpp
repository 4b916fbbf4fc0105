// The window pick of the one-pass method (onepass_pick_T_singlepass,
// horizon_selection.py:215-282) for one problem, shared by onepass.hip's pick kernel and
// the host test build (onepass_host.cpp, -DHOP_HD=).
//
// The reference collects the candidates' norms in a list, takes their median, sorts the
// candidates centre-out and scans them.  Here nothing is collected: pass 1 parks every
// candidate's norm in the output row Jw (candidate T owns Jw[T-1]), the median is found
// by counting ranks over those entries (at most 129 of them), and pass 2 walks the
// window centre-out, the smaller T first at equal distance, and replaces each parked norm
// by J_T, or by NaN where the locality gate removes the candidate.
#pragma once
#include <math.h>

#include "wrap.hpp"

namespace hop {
namespace onepass {

constexpr int kMaxWindow = 64;  // HOP_ONEPASS_MAX_WINDOW

struct PickDims {
  int n_ext;  // rows of X_ext, Vxx, Vx, V0
  int T_min, T_max, S_left, S_right;
  unsigned wrap_mask;
  double locality_mult;
};

HOP_HD inline bool pick_finite(double v) { return v - v == 0.0; }
// np.clip(v, lo, hi) = minimum(maximum(v, lo), hi)
HOP_HD inline int pick_clip(int v, int lo, int hi) {
  const int a = v > lo ? v : lo;
  return a < hi ? a : hi;
}
// a norm that enters the median (horizon_selection.py:260)
HOP_HD inline bool pick_counts(double dn) { return pick_finite(dn) && dn > 1e-12; }

template <int n>
HOP_HD inline double pick_dx0(const double* x0, const double* xi, unsigned mask, double* dx) {
  double ss = 0.0;
  for (int j = 0; j < n; ++j) {
    const double d = x0[j] - xi[j];
    dx[j] = (mask >> j) & 1u ? wrap_angle(d) : d;
    ss += dx[j] * dx[j];
  }
  return sqrt(ss);
}

// the k-th smallest (0-based) of the counted norms parked in Jw[lo-1 .. hi-1]
HOP_HD inline double pick_kth(const double* Jw, int lo, int hi, int k) {
  for (int T = lo; T <= hi; ++T) {
    const double v = Jw[T - 1];
    if (!pick_counts(v)) continue;
    int less = 0, leq = 0;
    for (int S = lo; S <= hi; ++S) {
      const double u = Jw[S - 1];
      if (!pick_counts(u)) continue;
      less += u < v;
      leq += u <= v;
    }
    if (less <= k && k < leq) return v;
  }
  return NAN;  // not reached for 0 <= k < count
}

// Vxx [n_ext][n][n], Vx [n_ext][n], V0 [n_ext], X_ext [n_ext][n], x0 [n] of one problem;
// writes Jw [T_max] and returns T*
template <int n>
HOP_HD inline int pick_one(const PickDims& d, const double* Vxx, const double* Vx,
                           const double* V0, const double* X_ext, const double* x0, int T_bar,
                           double* Jw) {
  for (int k = 0; k < d.T_max; ++k) Jw[k] = NAN;
  const int L = d.T_min > T_bar - d.S_left ? d.T_min : T_bar - d.S_left;
  const int R = d.T_max < T_bar + d.S_right ? d.T_max : T_bar + d.S_right;
  if (L > R) return pick_clip(T_bar, d.T_min, d.T_max);
  double dx[n];
  // pass 1: the norms
  int count = 0;
  for (int T = L; T <= R; ++T) {
    const int i = T_bar - T + d.S_right;
    if (i < 0 || i >= d.n_ext) continue;
    const double dn = pick_dx0<n>(x0, X_ext + (long long)i * n, d.wrap_mask, dx);
    Jw[T - 1] = dn;
    count += pick_counts(dn);
  }
  double dx_max = INFINITY;
  if (count > 0) {
    const double lo = pick_kth(Jw, L, R, (count - 1) / 2);
    // np.median: the middle value, or the mean of the two middle values
    const double med = (count & 1) ? lo : (lo + pick_kth(Jw, L, R, count / 2)) / 2.0;
    dx_max = d.locality_mult * med;
  }
  // pass 2: centre-out
  double bestJ = INFINITY;
  int bestT = pick_clip(T_bar, L, R);
  const int dl = T_bar - L, dr = R - T_bar;
  const int dmax = dl > dr ? dl : dr;
  for (int dist = 0; dist <= dmax; ++dist) {
    for (int side = 0; side < (dist ? 2 : 1); ++side) {
      const int T = side ? T_bar + dist : T_bar - dist;
      if (T < L || T > R) continue;
      const int i = T_bar - T + d.S_right;
      if (i < 0 || i >= d.n_ext) continue;
      pick_dx0<n>(x0, X_ext + (long long)i * n, d.wrap_mask, dx);
      const double dn = Jw[T - 1];  // the norm the median saw
      if (dn > dx_max) {
        Jw[T - 1] = NAN;
        continue;
      }
      const double* M = Vxx + (long long)i * n * n;
      const double* g = Vx + (long long)i * n;
      double quad = 0.0, lin = 0.0;
      for (int r = 0; r < n; ++r) {
        double row = 0.0;
        for (int c = 0; c < n; ++c) row += M[r * n + c] * dx[c];
        quad += dx[r] * row;
        lin += g[r] * dx[r];
      }
      const double JT = 0.5 * quad + lin + V0[i];
      Jw[T - 1] = JT;
      if (JT < bestJ) {
        bestJ = JT;
        bestT = T;
      }
    }
  }
  if (!pick_finite(bestJ)) bestT = pick_clip(T_bar, L, R);
  return bestT;
}

}  // namespace onepass
}  // namespace hop
