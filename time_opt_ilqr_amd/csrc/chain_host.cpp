// Host build of chain_dynamics.hpp for the CPU test suite (not part of libhop_amd.so):
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-builtin-sin -shared -fPIC -DHOP_HD=
//       chain_host.cpp -o libchain_host.so
// Runs chain.hip's per-step arithmetic (the base springs, the moved springs of every
// q column, then every entry of [A | B] from them) on the CPU, step by step, so the CPU
// tests hold it to the NumPy chain and host_dynamics.linearize.
#include <stdint.h>

#include "chain_dynamics.hpp"

using namespace hop::chain;

static bool params_ok(const Params& P) {
  return P.p >= 1 && P.p <= kMaxP && P.m >= 1 && P.m <= P.p;
}

template <bool CEN>
static void lin_run(const Params& P, const double* X, const double* U, int64_t batch, int nalloc,
                    int nuse, double epsx, double epsu, double relx, double relu, double* A,
                    double* B, double* a_res, double* Fx) {
  const int p = P.p, n = 2 * p, m = P.m;
  int jact[kMaxP];
  for (int a = 0; a < p; ++a) jact[a] = 0;
  for (int j = 0; j < m; ++j) jact[act_mass(j, p, m)] = j + 1;
  for (int64_t b = 0; b < batch; ++b)
    for (int k = 0; k < nuse; ++k) {
      const int64_t r = b * nalloc + k, xr = r + b;
      const double* x = X + xr * n;
      const double* u = U + r * m;
      double f0[kMaxP + 1], fm[4 * kMaxP], F0[kMaxN];
      springs(P, x, f0);
      for (int j = 0; j < p; ++j) {
        const double h = fd_step(x[j], epsx, relx);
        for (int s = 0; s < (CEN ? 4 : 2); ++s) fm[4 * j + s] = moved_spring(P, x, j, s, h);
      }
      bool fin = true;
      for (int i = 0; i < n; ++i) {
        F0[i] = chain_out(P, x, u, f0, fm, jact, i, -1, 0, 0.0);
        fin = fin && finite_d(F0[i]);
        if (a_res) a_res[r * n + i] = F0[i] - X[(xr + 1) * n + i];
        if (Fx) Fx[r * n + i] = F0[i];
      }
      for (int jj = 0; jj < n + m; ++jj) {
        const double h = col_step(P, x, u, jj, epsx, epsu, relx, relu);
        for (int i = 0; i < n; ++i) {
          const double v = fd_entry<CEN>(P, x, u, f0, fm, jact, F0, fin, i, jj, h);
          if (jj < n) A[r * n * n + i * n + jj] = v;
          else B[r * n * m + i * m + (jj - n)] = v;
        }
      }
    }
}

extern "C" {

// F at `count` (x, u) rows
int chain_host_dynamics(int p, int m, double dt, double k, double ks, double c, const double* X,
                        const double* U, int64_t count, double* Xn) {
  const Params P{p, m, dt, k, ks, c};
  if (!params_ok(P)) return -2;
  for (int64_t r = 0; r < count; ++r) eval(P, X + r * 2 * p, U + r * m, Xn + r * 2 * p);
  return 0;
}

int chain_host_linearize(int p, int m, double dt, double k, double ks, double c, const double* X,
                         const double* U, int64_t batch, int nalloc, int nuse, int central,
                         double epsx, double epsu, double relx, double relu, double* A, double* B,
                         double* a_res, double* Fx) {
  const Params P{p, m, dt, k, ks, c};
  if (!params_ok(P)) return -2;
  if (central) lin_run<true>(P, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
  else lin_run<false>(P, X, U, batch, nalloc, nuse, epsx, epsu, relx, relu, A, B, a_res, Fx);
  return 0;
}

}  // extern "C"
