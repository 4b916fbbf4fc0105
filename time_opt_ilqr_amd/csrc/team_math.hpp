// A team's per-member arithmetic (include/hop_team.h), shared by team.hip and the host
// test build (team_host.cpp): up to 15 members, each one of dynamics.hpp's systems and
// each of its own kind, stacked member-major.  Member a owns states [xo, xo + n_s) and
// inputs [uo, uo + m_s), xo and uo the running sums of the sizes before it; F is the
// concatenation of the members' F, so a team step is dyn::eval per member and the
// linearisation's diagonal blocks are dyn::fd_col's columns (linearize.hip's own sequence:
// the trig jobs, f0 from the base trig, then the columns).  The base point of a member
// does not depend on where the member sits: it is fleet_math.hpp's member_base.
//
// Off the diagonal blocks the rule is fleet_math.hpp's:
//   central  (F_i - F_i) / (2 h): 0.0, NaN where output i of F is not finite
//   forward  the whole (A_k, B_k) NaN when f0 is not finite in any member, else 0.0
#pragma once
#include <stdint.h>

#include "fleet_math.hpp"

namespace hop {
namespace team {

using namespace hop::dyn;
using fleet::kMaxM;
using fleet::kMaxN;
using fleet::member_base;
using fleet::MemberBase;

constexpr int kMaxMembers = 15;  // HOP_TEAM_MAX_MEMBERS

// A team's composition: the sizes, and per member the kind (3 bits), the state offset
// (5 bits) and the input offset (4 bits) packed by member index, so that a lane decodes
// its own with shifts by its lane index and nothing is indexed at run time.
struct Shape {
  int count, n, m;
  bool quad;              // a quadrotor among the members: the <12, 4> instantiation
  uint64_t kind, uo;      // member a: bits [3 a, 3 a + 3), [4 a, 4 a + 4)
  uint64_t xo_lo, xo_hi;  // members 0..7 and 8..14: bits [5 (a & 7), 5 (a & 7) + 5)
};

HOP_HD inline int kind_of(const Shape& s, int a) { return (int)((s.kind >> (3 * a)) & 7u); }
HOP_HD inline int xo_of(const Shape& s, int a) {
  return (int)(((a < 8 ? s.xo_lo : s.xo_hi) >> (5 * (a & 7))) & 31u);
}
HOP_HD inline int uo_of(const Shape& s, int a) { return (int)((s.uo >> (4 * a)) & 15u); }

// 0, or which limit the composition breaks: 1 count outside 1..15, 2 an unknown member
// id, 3 n > 31 or m > 16
inline int shape_of(int count, const int32_t* system, Shape* out) {
  if (count < 1 || count > kMaxMembers) return 1;
  Shape s{count, 0, 0, false, 0, 0, 0, 0};
  for (int a = 0; a < count; ++a) {
    const int k = system[a];
    if (k < 0 || k >= kNumSystems) return 2;
    if (s.n + state_dim(k) > kMaxN || s.m + control_dim(k) > kMaxM) return 3;
    s.kind |= (uint64_t)k << (3 * a);
    s.uo |= (uint64_t)s.m << (4 * a);
    (a < 8 ? s.xo_lo : s.xo_hi) |= (uint64_t)s.n << (5 * (a & 7));
    s.quad = s.quad || k == kQuadrotor;
    s.n += state_dim(k), s.m += control_dim(k);
  }
  *out = s;
  return 0;
}

// Rows [xo, xo + n_s) of A_k [n][n] and B_k [n][m] of the team: the member's block from
// fd_col, the rest of the rows from the rule above.  team_fin: f0 is finite in every
// member (the forward form's test).
template <int SYS, bool CEN>
HOP_HD inline void member_rows(int xo, int uo, int n, int m, const double* x, const double* u,
                               const MemberBase<SYS, CEN>& b, bool team_fin, double dt,
                               double epsx, double epsu, double relx, double relu, double* A,
                               double* B) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < ns; ++i) {
    const double off = (CEN ? finite_d(b.f0[i]) : team_fin) ? 0.0 : nan;
    double* Ar = A + (xo + i) * n;
    double* Br = B + (xo + i) * m;
    for (int c = 0; c < n; ++c)
      if (c < xo || c >= xo + ns) Ar[c] = off;
    for (int c = 0; c < m; ++c)
      if (c < uo || c >= uo + ms) Br[c] = off;
  }
  for (int j = 0; j < ns + ms; ++j) {
    double col[ns];
    fd_col<SYS, CEN>(x, u, b.f0, CEN ? b.fin : team_fin, b.ts, dt, j, epsx, epsu, relx, relu,
                     col);
#pragma unroll
    for (int i = 0; i < ns; ++i) {
      if (j < ns) A[(xo + i) * n + xo + j] = col[i];
      else B[(xo + i) * m + uo + (j - ns)] = col[i];
    }
  }
}

}  // namespace team
}  // namespace hop
