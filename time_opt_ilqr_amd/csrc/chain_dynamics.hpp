// Discrete-time dynamics of the mass-spring chain (tests/golden/make_golden_wide.py
// chain_dynamics) and the entries of its finite-difference Jacobians, for the device
// kernels (chain.hip) and the host test build (chain_host.cpp).
//   x = [q (p positions), v (p velocities)], n = 2 p <= 30, u [m], 1 <= m <= p <= 15
//   unit masses between two fixed ends; spring i (0 <= i <= p) joins mass i - 1 and
//   mass i, the walls being q_{-1} = q_p = 0
//     d_i   = q_i - q_{i-1}                        ext = [0, q, 0]; d = diff(ext)
//     f_i   = (k d_i) + (ks sin d_i)
//     acc_i = (f_{i+1} - f_i) - c v_i, then += u_j on mass j * p // m
//     q'    = q + dt v,  v' = v + dt acc           explicit Euler
// The size is a run-time argument.  Expressions follow the NumPy order and are compiled
// without FMA contraction (HOP_DYN_BEGIN), so sin is the only operation that can differ
// from NumPy: the q' half of F is bit-identical.
//
// Locality of the Jacobian: column q_j moves springs j and j + 1 only, column v_j moves
// q'_j and v'_j, column u_j moves v'_act(j).  chain_out evaluates ONE output of F at a
// point moved along one column from the springs of the base point and the (at most
// four) moved springs of that column; an output the column does not reach is then the
// same number on both sides of the quotient, an exact zero (NaN when it is not finite),
// as in the reference, which evaluates all of F.
#pragma once
#include <math.h>

#include "dynamics.hpp"

namespace hop {
namespace chain {

using hop::dyn::fd_step;
using hop::dyn::finite_d;

constexpr int kMaxP = 15;            // masses: p + 1 <= 16 springs, one DPP row
constexpr int kMaxN = 2 * kMaxP;     // states

struct Params {
  int p, m;
  double dt, k, ks, c;
};

HOP_HD inline int act_mass(int j, int p, int m) { return j * p / m; }  // j * p // m

// spring force on the stretch d
HOP_HD inline double spring(double d, double k, double ks) {
  HOP_DYN_BEGIN
  return (k * d) + (ks * sin(d));
}

// stretch of spring i from the positions on either side (hi = q_i, lo = q_{i-1})
HOP_HD inline double stretch(double hi, double lo) {
  HOP_DYN_BEGIN
  return hi - lo;
}

HOP_HD inline double q_next(double q, double v, double dt) {
  HOP_DYN_BEGIN
  return q + dt * v;
}

// v' of one mass: fhi = f_{i+1}, flo = f_i; u is added only on an actuated mass
HOP_HD inline double v_next(double v, double fhi, double flo, double c, double dt, bool has_u,
                            double u) {
  HOP_DYN_BEGIN
  double acc = (fhi - flo) - c * v;
  if (has_u) acc += u;
  return v + dt * acc;
}

// all p + 1 springs of x
HOP_HD inline void springs(const Params& P, const double* x, double* f) {
  for (int i = 0; i <= P.p; ++i)
    f[i] = spring(stretch(i < P.p ? x[i] : 0.0, i > 0 ? x[i - 1] : 0.0), P.k, P.ks);
}

// the whole of F (host tests, the single-step kernel)
HOP_HD inline void eval(const Params& P, const double* x, const double* u, double* o) {
  const int p = P.p;
  double f[kMaxP + 1];
  springs(P, x, f);
  for (int i = 0; i < p; ++i) {
    int ja = -1;
    for (int j = 0; j < P.m; ++j)
      if (act_mass(j, p, P.m) == i) ja = j;
    o[i] = q_next(x[i], x[p + i], P.dt);
    o[p + i] = v_next(x[p + i], f[i + 1], f[i], P.c, P.dt, ja >= 0, ja >= 0 ? u[ja] : 0.0);
  }
}

// ---- finite differences (linearization.py:177-262) ---------------------------
// h of column jj (jj < n: x_jj, else u_{jj-n})
HOP_HD inline double col_step(const Params& P, const double* x, const double* u, int jj,
                              double epsx, double epsu, double relx, double relu) {
  const int n = 2 * P.p;
  return jj < n ? fd_step(x[jj], epsx, relx) : fd_step(u[jj - n], epsu, relu);
}

// The moved springs of column q_j: slot 2 * sgn + hi, sgn 0: q_j + h, 1: q_j - h;
// hi 0: spring j, 1: spring j + 1.  Four per column (central), two (forward).
HOP_HD inline double moved_spring(const Params& P, const double* x, int j, int slot, double h) {
  HOP_DYN_BEGIN
  const int p = P.p;
  const double qj = (slot >> 1) ? x[j] - h : x[j] + h;
  const double d = (slot & 1) ? stretch(j + 1 < p ? x[j + 1] : 0.0, qj)
                              : stretch(qj, j > 0 ? x[j - 1] : 0.0);
  return spring(d, P.k, P.ks);
}

// Output i of F at the point moved by +h (sgn 0) or -h (sgn 1) along column jj (jj < 0:
// the base point).  f0: the p + 1 base springs; fm: the moved springs [p][4]; jact[a]:
// 1 + the input that pushes mass a, or 0 (so that the table, which the kernel keeps in
// LDS, holds no all-ones words: read as doubles they would be NaN bit patterns).
HOP_HD inline double chain_out(const Params& P, const double* x, const double* u,
                               const double* f0, const double* fm, const int* jact, int i,
                               int jj, int sgn, double h) {
  HOP_DYN_BEGIN
  const int p = P.p, n = 2 * p;
  if (i < p) {
    double q = x[i], v = x[p + i];
    if (jj == i) q = sgn ? q - h : q + h;
    if (jj == p + i) v = sgn ? v - h : v + h;
    return q_next(q, v, P.dt);
  }
  const int a = i - p;
  double v = x[p + a], flo = f0[a], fhi = f0[a + 1];
  if (jj >= 0 && jj < p) {
    if (jj == a) flo = fm[jj * 4 + 2 * sgn], fhi = fm[jj * 4 + 2 * sgn + 1];
    else if (jj == a - 1) flo = fm[jj * 4 + 2 * sgn + 1];  // spring a is its spring j + 1
    else if (jj == a + 1) fhi = fm[jj * 4 + 2 * sgn];      // spring a + 1 is its spring j
  } else if (jj == p + a) {
    v = sgn ? v - h : v + h;
  }
  const int ja = jact[a] - 1;
  double ua = 0.0;
  if (ja >= 0) {
    ua = u[ja];
    if (jj == n + ja) ua = sgn ? ua - h : ua + h;
  }
  return v_next(v, fhi, flo, P.c, P.dt, ja >= 0, ua);
}

// true when column jj can move output i of F
HOP_HD inline bool reaches(const Params& P, const int* jact, int i, int jj) {
  const int p = P.p, n = 2 * p;
  if (i < p) return jj == i || jj == p + i;
  const int a = i - p;
  if (jj < p) return jj >= a - 1 && jj <= a + 1;
  return jj == p + a || (jj >= n && jj - n == jact[a] - 1);
}

// Entry (i, jj) of [A | B]:
//   central  (F_i(v + h e) - F_i(v - h e)) / (2 h)     linearization.py:195-208
//   forward  (F_i(v + h e) - F_i(v)) / h, NaN when F(x, u) is not finite (241-258)
// Where the column does not reach the output both sides of the quotient are F0[i], and
// (F0[i] - F0[i]) / (a positive h) is +0.0 for a finite F0[i] and NaN otherwise: written
// without the two evaluations and the division.
template <bool CEN>
HOP_HD inline double fd_entry(const Params& P, const double* x, const double* u, const double* f0,
                              const double* fm, const int* jact, const double* F0,
                              bool f0_finite, int i, int jj, double h) {
  HOP_DYN_BEGIN
  if (!CEN && !f0_finite) return __builtin_nan("");
  if (!reaches(P, jact, i, jj)) return finite_d(F0[i]) ? 0.0 : __builtin_nan("");
  if constexpr (CEN) {
    const double fp = chain_out(P, x, u, f0, fm, jact, i, jj, 0, h);
    const double fn = chain_out(P, x, u, f0, fm, jact, i, jj, 1, h);
    return (fp - fn) / (2.0 * h);
  } else {
    if (!f0_finite) return __builtin_nan("");
    const double fp = chain_out(P, x, u, f0, fm, jact, i, jj, 0, h);
    return (fp - F0[i]) / h;
  }
}

}  // namespace chain
}  // namespace hop
