// A fleet's per-member arithmetic (include/hop_fleet.h), shared by fleet.hip and the
// host test build (fleet_host.cpp): `count` copies of one system of dynamics.hpp, stacked
// member-major.  Member a owns states [a n_s, (a + 1) n_s) and inputs [a m_s, (a + 1) m_s);
// F is the concatenation of the members' F, so a fleet step is dyn::eval per member and
// the linearisation's diagonal blocks are dyn::fd_col's columns (linearize.hip's own
// sequence: the trig jobs, f0 from the base trig, then the columns).
//
// Off the diagonal blocks the reference's finite differences on the stacked callable
// subtract a number from itself (the other members are not moved by the column's step):
//   central  (F_i - F_i) / (2 h): 0.0, NaN where output i of F is not finite
//   forward  (F_i - f0_i) / h with the whole (A_k, B_k) NaN when f0 is not finite
//            in any member (linearization.py:245-250), else 0.0
#pragma once
#include "dynamics.hpp"

namespace hop {
namespace fleet {

using namespace hop::dyn;

constexpr int kMaxN = 31, kMaxM = 16;  // HOP_FLEET_MAX_N, HOP_FLEET_MAX_M

// (count, n, m) fit the wide path
HOP_HD inline bool shape_ok(int sys, int count) {
  return sys >= 0 && sys < kNumSystems && count >= 1 && count <= kMaxN &&
         count * state_dim(sys) <= kMaxN && count * control_dim(sys) <= kMaxM;
}

template <int SYS, bool CEN>
struct MemberBase {
  static constexpr int n = state_dim(SYS);
  static constexpr int TS = trig_slots(SYS, CEN) > 0 ? trig_slots(SYS, CEN) : 1;
  double ts[TS];  // the quadrotor's trig slots (dynamics.hpp), unused otherwise
  double f0[n];   // F(x, u) of this member
  bool fin;       // f0 finite
};

// the base point of one member at one step: linearize.hip's phases 1 and 2
template <int SYS, bool CEN>
HOP_HD inline void member_base(const double* x, const double* u, double dt, double epsx,
                               double relx, MemberBase<SYS, CEN>& b) {
  constexpr int n = state_dim(SYS);
#pragma unroll
  for (int i = 0; i < MemberBase<SYS, CEN>::TS; ++i) b.ts[i] = 0.0;
  for (int job = 0; job < trig_jobs(SYS, CEN); ++job) quad_trig_job(x, job, epsx, relx, b.ts);
  if constexpr (SYS == kQuadrotor)
    f_quadrotor_t(x, u, dt,
                  QuadTrig{b.ts[0], b.ts[1], b.ts[2], b.ts[3], b.ts[4], b.ts[5], b.ts[6]}, b.f0);
  else
    eval<SYS>(x, u, dt, b.f0);
  b.fin = true;
#pragma unroll
  for (int i = 0; i < n; ++i) b.fin = b.fin && finite_d(b.f0[i]);
}

// Rows [a n_s, (a + 1) n_s) of A_k [n][n] and B_k [n][m] of the fleet: member a's block
// from fd_col, the rest of the rows from the rule above.  fleet_fin: f0 is finite in
// every member (the forward form's test).
template <int SYS, bool CEN>
HOP_HD inline void member_rows(int a, int count, const double* x, const double* u,
                               const MemberBase<SYS, CEN>& b, bool fleet_fin, double dt,
                               double epsx, double epsu, double relx, double relu, double* A,
                               double* B) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const int n = count * ns, m = count * ms;
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < ns; ++i) {
    const double off = (CEN ? finite_d(b.f0[i]) : fleet_fin) ? 0.0 : nan;
    double* Ar = A + (a * ns + i) * n;
    double* Br = B + (a * ns + i) * m;
    for (int c = 0; c < n; ++c)
      if (c < a * ns || c >= (a + 1) * ns) Ar[c] = off;
    for (int c = 0; c < m; ++c)
      if (c < a * ms || c >= (a + 1) * ms) Br[c] = off;
  }
  for (int j = 0; j < ns + ms; ++j) {
    double col[ns];
    fd_col<SYS, CEN>(x, u, b.f0, CEN ? b.fin : fleet_fin, b.ts, dt, j, epsx, epsu, relx, relu,
                     col);
#pragma unroll
    for (int i = 0; i < ns; ++i) {
      if (j < ns) A[(a * ns + i) * n + a * ns + j] = col[i];
      else B[(a * ns + i) * m + a * ms + (j - ns)] = col[i];
    }
  }
}

}  // namespace fleet
}  // namespace hop
