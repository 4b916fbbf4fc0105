// Host build of team_math.hpp for the CPU test suite (not part of libhop_amd.so):
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-builtin-{sin,cos,tan} -shared -fPIC -DHOP_HD=
//       team_host.cpp -o libteam_host.so
// Runs team.hip's per-member arithmetic (the member's step, its base point, then rows
// [xo, xo + n_s) of [A | B]) on the CPU, member by member, so the CPU tests hold it to
// the members' host dynamics (dyn_host.cpp) and to host_dynamics.linearize on the stacked
// callable.  With -DTEAM_HOST_MAIN it is a stand-alone program that runs both functions
// over two teams (every kind in one row; eight members next to both size limits) and
// checks the blocks' structure: the build for -fsanitize=address,undefined.
#include <stdint.h>

#include "team_math.hpp"

using namespace hop::team;

// f<SYS>() for the member's kind
#define TEAM_KIND(kind, CALL)                 \
  switch (kind) {                             \
    case kDI: CALL(kDI); break;               \
    case kCartpole: CALL(kCartpole); break;   \
    case kQuadrotor: CALL(kQuadrotor); break; \
    case kPointmass: CALL(kPointmass); break; \
    default: CALL(kSegway); break;            \
  }

// every kind's base point, one of them filled per member
template <bool CEN>
struct AnyBase {
  MemberBase<kDI, CEN> di;
  MemberBase<kCartpole, CEN> cp;
  MemberBase<kQuadrotor, CEN> quad;
  MemberBase<kPointmass, CEN> pm;
  MemberBase<kSegway, CEN> seg;
  template <int SYS>
  MemberBase<SYS, CEN>& of() {
    if constexpr (SYS == kDI) return di;
    else if constexpr (SYS == kCartpole) return cp;
    else if constexpr (SYS == kQuadrotor) return quad;
    else if constexpr (SYS == kPointmass) return pm;
    else return seg;
  }
};

template <bool CEN>
static void lin_run(const Shape& s, double dt, const double* X, const double* U, int64_t batch,
                    int nalloc, int nuse, double epsx, double epsu, double relx, double relu,
                    double* A, double* B, double* a_res, double* Fx) {
  const int n = s.n, m = s.m;
  for (int64_t b = 0; b < batch; ++b)
    for (int k = 0; k < nuse; ++k) {
      const int64_t r = b * nalloc + k, xr = r + b;
      AnyBase<CEN> mb[kMaxMembers];
      bool team_fin = true;
      for (int a = 0; a < s.count; ++a) {
        const double* x = X + xr * n + xo_of(s, a);
        const double* u = U + r * m + uo_of(s, a);
#define TEAM_BASE(S)                                                               \
  member_base<S, CEN>(x, u, dt, epsx, relx, mb[a].template of<S>());               \
  team_fin = team_fin && mb[a].template of<S>().fin
        TEAM_KIND(kind_of(s, a), TEAM_BASE)
#undef TEAM_BASE
      }
      for (int a = 0; a < s.count; ++a) {
        const int xo = xo_of(s, a), uo = uo_of(s, a);
        const double* x = X + xr * n + xo;
        const double* u = U + r * m + uo;
#define TEAM_ROWS(S)                                                               \
  {                                                                                \
    const MemberBase<S, CEN>& g = mb[a].template of<S>();                          \
    for (int i = 0; i < state_dim(S); ++i) {                                       \
      const int64_t o = r * n + xo + i;                                            \
      if (a_res) a_res[o] = g.f0[i] - X[(xr + 1) * n + xo + i];                    \
      if (Fx) Fx[o] = g.f0[i];                                                     \
    }                                                                              \
    member_rows<S, CEN>(xo, uo, n, m, x, u, g, team_fin, dt, epsx, epsu, relx, relu, \
                        A + r * n * n, B + r * n * m);                             \
  }
        TEAM_KIND(kind_of(s, a), TEAM_ROWS)
#undef TEAM_ROWS
      }
    }
}

extern "C" {

// (n, m) of the team, or the code of team_math.hpp's shape_of (1 count, 2 member, 3 size)
int team_host_shape(int count, const int32_t* system, int* n, int* m) {
  Shape s;
  if (int rc = shape_of(count, system, &s)) return rc;
  *n = s.n, *m = s.m;
  return 0;
}

// F of the stacked system at `rows` (x, u) rows
int team_host_dynamics(int count, const int32_t* system, double dt, const double* X,
                       const double* U, int64_t rows, double* Xn) {
  Shape s;
  if (shape_of(count, system, &s)) return -2;
  for (int64_t r = 0; r < rows; ++r)
    for (int a = 0; a < s.count; ++a) {
      const int xo = xo_of(s, a), uo = uo_of(s, a);
#define TEAM_STEP(S) eval<S>(X + r * s.n + xo, U + r * s.m + uo, dt, Xn + r * s.n + xo)
      TEAM_KIND(kind_of(s, a), TEAM_STEP)
#undef TEAM_STEP
    }
  return 0;
}

int team_host_linearize(int count, const int32_t* system, double dt, const double* X,
                        const double* U, int64_t batch, int nalloc, int nuse, int central,
                        double epsx, double epsu, double relx, double relu, double* A, double* B,
                        double* a_res, double* Fx) {
  Shape s;
  if (shape_of(count, system, &s)) return -2;
  if (central)
    lin_run<true>(s, dt, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
  else
    lin_run<false>(s, dt, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
  return 0;
}

}  // extern "C"

#ifdef TEAM_HOST_MAIN
#include <stdio.h>

#include <vector>

// one team: a short batch of trajectories from a fixed generator through the step and
// both linearisation forms, in buffers of exactly the documented sizes
static int run_team(const char* tag, int count, const int32_t* system, double dt) {
  int n = 0, m = 0;
  if (team_host_shape(count, system, &n, &m)) return printf("%s: bad shape\n", tag), 1;
  const int B = 3, N = 5;
  std::vector<double> X((size_t)B * (N + 1) * n), U((size_t)B * N * m);
  uint64_t st = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() {  // uniform in [-0.5, 0.5)
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(st >> 11) / 9007199254740992.0 - 0.5;
  };
  for (double& v : U) v = rnd();
  for (int b = 0; b < B; ++b) {
    double* x = X.data() + (size_t)b * (N + 1) * n;
    for (int i = 0; i < n; ++i) x[i] = rnd();
    for (int k = 0; k < N; ++k)
      if (team_host_dynamics(count, system, dt, x + (size_t)k * n,
                             U.data() + ((size_t)b * N + k) * m, 1, x + (size_t)(k + 1) * n))
        return printf("%s: dynamics failed\n", tag), 1;
  }
  std::vector<int> owner(n, -1), uowner(m, -1);  // which member owns a state / an input
  for (int a = 0, x = 0, u = 0; a < count; ++a) {
    for (int i = 0; i < state_dim(system[a]); ++i) owner[x++] = a;
    for (int i = 0; i < control_dim(system[a]); ++i) uowner[u++] = a;
  }
  int bad = 0;
  for (int central = 0; central < 2; ++central) {
    std::vector<double> A((size_t)B * N * n * n, -7.0), Bm((size_t)B * N * n * m, -7.0);
    std::vector<double> ar((size_t)B * N * n, -7.0), fx((size_t)B * N * n, -7.0);
    if (team_host_linearize(count, system, dt, X.data(), U.data(), B, N, N - 1, central, 1e-5,
                            1e-5, 1e-6, 1e-6, A.data(), Bm.data(), ar.data(), fx.data()))
      return printf("%s: linearize failed\n", tag), 1;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k) {
        const size_t r = (size_t)b * N + k;
        for (int i = 0; i < n; ++i) {
          const bool written = k < N - 1;  // n_use = N - 1: the last step stays untouched
          for (int c = 0; c < n; ++c) {
            const double v = A[(r * n + i) * n + c];
            if (!written) bad += v != -7.0;
            else if (owner[i] != owner[c]) bad += !(v == 0.0);
            else bad += !(v == v) || v == -7.0;
          }
          for (int c = 0; c < m; ++c) {
            const double v = Bm[(r * n + i) * m + c];
            if (!written) bad += v != -7.0;
            else if (owner[i] != uowner[c]) bad += !(v == 0.0);
            else bad += !(v == v) || v == -7.0;
          }
          // the rollout above is this very arithmetic: its residual is an exact zero
          bad += written ? !(ar[r * n + i] == 0.0) || fx[r * n + i] != X[((size_t)b * (N + 1) + k + 1) * n + i]
                         : ar[r * n + i] != -7.0 || fx[r * n + i] != -7.0;
        }
      }
  }
  printf("%s: n = %d, m = %d, %d members, %d bad entries\n", tag, n, m, count, bad);
  return bad != 0;
}

int main() {
  const int32_t all5[] = {0, 1, 2, 3, 4};
  const int32_t pm7_di[] = {3, 3, 3, 3, 3, 3, 3, 0};
  int rc = run_team("all5", 5, all5, 0.02);
  rc |= run_team("pm7_di", 8, pm7_di, 0.05);
  printf(rc ? "FAILED\n" : "OK\n");
  return rc;
}
#endif
