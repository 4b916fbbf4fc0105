// Host build of fleet_math.hpp for the CPU test suite (not part of libhop_amd.so):
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-builtin-{sin,cos,tan} -shared -fPIC -DHOP_HD=
//       fleet_host.cpp -o libfleet_host.so
// Runs fleet.hip's per-member arithmetic (the member's step, its base point, then rows
// [a n_s, (a + 1) n_s) of [A | B]) on the CPU, member by member, so the CPU tests hold it
// to the members' host dynamics (dyn_host.cpp) and to host_dynamics.linearize on the
// stacked callable.
#include <stdint.h>

#include "fleet_math.hpp"

using namespace hop::fleet;

template <int SYS>
static void dyn_run(int count, double dt, const double* X, const double* U, int64_t rows,
                    double* Xn) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const int n = count * ns, m = count * ms;
  for (int64_t r = 0; r < rows; ++r)
    for (int a = 0; a < count; ++a)
      eval<SYS>(X + r * n + a * ns, U + r * m + a * ms, dt, Xn + r * n + a * ns);
}

template <int SYS, bool CEN>
static void lin_run(int count, double dt, const double* X, const double* U, int64_t batch,
                    int nalloc, int nuse, double epsx, double epsu, double relx, double relu,
                    double* A, double* B, double* a_res, double* Fx) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const int n = count * ns, m = count * ms;
  for (int64_t b = 0; b < batch; ++b)
    for (int k = 0; k < nuse; ++k) {
      const int64_t r = b * nalloc + k, xr = r + b;
      MemberBase<SYS, CEN> mb[kMaxN];
      bool fleet_fin = true;
      for (int a = 0; a < count; ++a) {
        member_base<SYS, CEN>(X + xr * n + a * ns, U + r * m + a * ms, dt, epsx, relx, mb[a]);
        fleet_fin = fleet_fin && mb[a].fin;
      }
      for (int a = 0; a < count; ++a) {
        for (int i = 0; i < ns; ++i) {
          const int64_t o = r * n + a * ns + i;
          if (a_res) a_res[o] = mb[a].f0[i] - X[(xr + 1) * n + a * ns + i];
          if (Fx) Fx[o] = mb[a].f0[i];
        }
        member_rows<SYS, CEN>(a, count, X + xr * n + a * ns, U + r * m + a * ms, mb[a], fleet_fin,
                              dt, epsx, epsu, relx, relu, A + r * n * n, B + r * n * m);
      }
    }
}

template <int SYS>
static void lin_sys(int central, int count, double dt, const double* X, const double* U,
                    int64_t batch, int nalloc, int nuse, double epsx, double epsu, double relx,
                    double relu, double* A, double* B, double* a_res, double* Fx) {
  if (central)
    lin_run<SYS, true>(count, dt, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
  else
    lin_run<SYS, false>(count, dt, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
}

extern "C" {

// F of the stacked system at `rows` (x, u) rows
int fleet_host_dynamics(int sys, int count, double dt, const double* X, const double* U,
                        int64_t rows, double* Xn) {
  if (!shape_ok(sys, count)) return -2;
  switch (sys) {
    case kDI: dyn_run<kDI>(count, dt, X, U, rows, Xn); break;
    case kCartpole: dyn_run<kCartpole>(count, dt, X, U, rows, Xn); break;
    case kQuadrotor: dyn_run<kQuadrotor>(count, dt, X, U, rows, Xn); break;
    case kPointmass: dyn_run<kPointmass>(count, dt, X, U, rows, Xn); break;
    default: dyn_run<kSegway>(count, dt, X, U, rows, Xn); break;
  }
  return 0;
}

int fleet_host_linearize(int sys, int count, double dt, const double* X, const double* U,
                         int64_t batch, int nalloc, int nuse, int central, double epsx,
                         double epsu, double relx, double relu, double* A, double* B,
                         double* a_res, double* Fx) {
  if (!shape_ok(sys, count)) return -2;
#define HOP_FLEET_LIN(S) \
  lin_sys<S>(central, count, dt, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx)
  switch (sys) {
    case kDI: HOP_FLEET_LIN(kDI); break;
    case kCartpole: HOP_FLEET_LIN(kCartpole); break;
    case kQuadrotor: HOP_FLEET_LIN(kQuadrotor); break;
    case kPointmass: HOP_FLEET_LIN(kPointmass); break;
    default: HOP_FLEET_LIN(kSegway); break;
  }
#undef HOP_FLEET_LIN
  return 0;
}

}  // extern "C"
