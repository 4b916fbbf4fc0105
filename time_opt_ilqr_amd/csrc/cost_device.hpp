// The true cost's device helpers (cost_timeopt_true, solver.py:65-102), shared by
// forward.hip and onepass.hip: the wrapped error, 0.5 v.(M v), the obstacle penalty,
// the running-cost increment of one step and the terminal term.  The cost follows the
// reference's evaluation order per step, c += (0.5 e.Qe + 0.5 du.Rdu) + w, then + c_extra.
#pragma once
#include <math.h>

#include "hop_kernels.hpp"
#include "dynamics.hpp"

namespace hop {
namespace fwd {

using namespace hop::dyn;

__device__ inline bool fin(double v) { return v - v == 0.0; }

// 0.5 v.(M v) for a row-major k x k matrix M (reference: 0.5 * float(v @ (M @ v)))
template <int K>
__device__ inline double half_quad(const double* __restrict__ M, const double* v) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) r = fma(M[i * K + j], v[j], r);
    acc = fma(v[i], r, acc);
  }
  return 0.5 * acc;
}

// the same for a diagonal M (off-diagonal entries exactly 0): the dense chain's
// fma(0, v_j, r) terms add exact zeros, so this is bitwise the same number
template <int K>
__device__ inline double half_quad_diag(const double* __restrict__ M, const double* v) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) acc = fma(v[i], M[i * K + i] * v[i], acc);
  return 0.5 * acc;
}

// sum of the Gaussian obstacle penalties at position (px, py) (systems.py:271-293, c only)
__device__ inline double obstacle_c(const double* __restrict__ obs, int n_obs, double px,
                                    double py) {
  double c = 0.0;
  for (int o = 0; o < n_obs; ++o) {
    const double dx = px - obs[4 * o], dy = py - obs[4 * o + 1], r = obs[4 * o + 2];
    const double s = dx * dx + dy * dy;
    c += obs[4 * o + 3] * exp(-s / (2.0 * r * r));
  }
  return c;
}

// WM >= 0: the wrap mask is a compile-time constant (the system's default
// wrap_idx), so unwrapped components cost nothing; WM = -1: runtime mask (every
// component's wrap is evaluated and selected)
template <int n, int WM = -1>
__device__ inline void wrap_err(const double* a, const double* b, unsigned mask, double* e) {
  const unsigned mk = WM >= 0 ? (unsigned)WM : mask;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const double d = a[i] - b[i];
    e[i] = (mk >> i) & 1u ? wrap_angle(d) : d;
  }
}

// running-cost increment of step k (solver.py:87-95); false if e or du is not finite
// SH: every cost block is shared by the batch (all batch strides 0), so the block
// addresses are wave-uniform and the compiler reads them through the scalar cache
// (stage_inc_e: the same with the wrapped error e given)
template <int n, int m, bool SH = false>
__device__ inline bool stage_inc_e(const CostArgs& c, long long b_, const double* x,
                                   const double* e, const double* u, double& acc, bool diag) {
  const long long b = SH ? 0 : b_;
  double du[m];
  const double* ur = c.u_ref + b * c.ur_bs;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < n; ++i) ok = ok && fin(e[i]);
#pragma unroll
  for (int i = 0; i < m; ++i) {
    du[i] = u[i] - ur[i];
    ok = ok && fin(du[i]);
  }
  const double q = diag ? half_quad_diag<n>(c.Q + b * c.q_bs, e) : half_quad<n>(c.Q + b * c.q_bs, e);
  const double r =
      diag ? half_quad_diag<m>(c.R + b * c.r_bs, du) : half_quad<m>(c.R + b * c.r_bs, du);
  acc += (q + r) + c.w[b * c.w_bs];
  if (c.obs) acc += obstacle_c(c.obs, c.n_obs, x[0], x[1]);
  return ok;
}

template <int n, int m, bool SH = false, int WM = -1>
__device__ inline bool stage_inc(const CostArgs& c, long long b_, const double* x,
                                 const double* u, double& acc, bool diag = false) {
  const long long b = SH ? 0 : b_;
  double e[n], du[m];
  wrap_err<n, WM>(x, c.xg + b * c.xg_bs, c.wrap_mask, e);
  const double* ur = c.u_ref + b * c.ur_bs;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < n; ++i) ok = ok && fin(e[i]);
#pragma unroll
  for (int i = 0; i < m; ++i) {
    du[i] = u[i] - ur[i];
    ok = ok && fin(du[i]);
  }
  const double q = diag ? half_quad_diag<n>(c.Q + b * c.q_bs, e) : half_quad<n>(c.Q + b * c.q_bs, e);
  const double r =
      diag ? half_quad_diag<m>(c.R + b * c.r_bs, du) : half_quad<m>(c.R + b * c.r_bs, du);
  acc += (q + r) + c.w[b * c.w_bs];
  if (c.obs) acc += obstacle_c(c.obs, c.n_obs, x[0], x[1]);
  return ok;
}

template <int n, bool SH = false, int WM = -1>
__device__ inline double terminal_cost(const CostArgs& c, long long b_, const double* x,
                                       bool& ok, bool diag = false) {
  const long long b = SH ? 0 : b_;
  double e[n];
  wrap_err<n, WM>(x, c.xg + b * c.xg_bs, c.wrap_mask, e);
#pragma unroll
  for (int i = 0; i < n; ++i) ok = ok && fin(e[i]);
  return diag ? half_quad_diag<n>(c.Qf + b * c.qf_bs, e) : half_quad<n>(c.Qf + b * c.qf_bs, e);
}

}  // namespace fwd
}  // namespace hop
