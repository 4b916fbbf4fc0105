// The one-pass window method (baseline2) on the device (include/hop_onepass.h):
//   nominal_cost_curve         solver.py:108-149, 537         hop_onepass_nominal_curve_f64
//   extend_nominal_backward    linearization.py:41-71, 109-170 hop_onepass_extend_backward_f64
//   onepass_pick_T_singlepass  horizon_selection.py:215-282   hop_onepass_pick_f64
//   onepass_rollout            solver.py:365-442              hop_onepass_rollout_f64
// The sweep between the prefix and the pick is hop_riccati_f64 mode 1.
//
// Everything here is sequential in time, so the parallelism is across problems: the
// curve, the prefix and the pick give one lane to a problem; the rollout gives one lane
// to every (problem, alpha) pair, as forward.hip's one-lane line search does, and a
// second pass (one workgroup per problem) takes the smallest J and copies its row.
// The dynamics are dynamics.hpp's eval<SYS>, the cost helpers cost_device.hpp's, the pick
// arithmetic onepass_pick.hpp's (also built for the host: onepass_host.cpp).
#include <math.h>

#include "hop_device.hpp"
#include "hop_kernels.hpp"
#include "dynamics.hpp"
#include "cost_device.hpp"
#include "onepass_pick.hpp"
#include "../../include/hop_onepass.h"

namespace hop {
namespace onepass {

using namespace hop::dyn;
using fwd::fin;

constexpr int TPB = 64;

struct CurveArgs {
  CostArgs c;
  const double* X; const double* U;       // [B][N+1][n], [B][N][m]
  long long batch; int N, T_min, T_max;
  double* J; int* T_bar;                  // [B][T_max], [B]
};
struct ExtendArgs {
  double dt;
  const double* X; const double* U;       // [B][N+1][n], [B][N][m]
  const double* u_fill;                   // [B][m]
  long long batch; int N, S, max_iter;
  double tol, damping;
  double* X_ext; double* U_ext;           // [B][S+N+1][n], [B][S+N][m]
};
struct PickArgs {
  PickDims d;
  const double* Vxx; const double* Vx; const double* V0;  // [B][n_ext][n][n], [..][n], [..]
  const double* X_ext; const double* x0;  // [B][n_ext][n], [B][n]
  const int* T_bar;
  long long batch;
  int* T_star; double* Jw;                // [B], [B][T_max]
};
struct RollArgs {
  CostArgs c;
  double dt;
  const double* X_ext; const double* U_ext;  // [B][S+N+1][n], [B][S+N][m]
  const int* T_bar; const int* T_star; const int* active;
  const double* K; const double* kff;        // [B][S+N][m][n], [B][S+N][m]
  double alphas[8]; int n_alpha;
  long long batch; int N, S;
  double* Jc;                                // workspace [B][n_alpha]
  double* ws;                                // workspace [B][n_alpha][(N+1)n + Nm]
  double* X_new; double* U_new; double* J; int* accepted;
};

// ---------------------------------------------------------------- nominal curve
template <int SYS>
__global__ __launch_bounds__(TPB) void curve_kernel(CurveArgs a) {
  constexpr int n = state_dim(SYS), m = control_dim(SYS);
  const long long b = (long long)blockIdx.x * TPB + threadIdx.x;
  if (b >= a.batch) return;
  const double* X = a.X + b * (long long)(a.N + 1) * n;
  const double* U = a.U + b * (long long)a.N * m;
  double* J = a.J + b * a.T_max;
  // solver.py:132: any non-finite value on the rows read gives the all-inf row
  bool all = true;
  for (int e = 0; e < (a.T_max + 1) * n; ++e) all = all && fin(X[e]);
  for (int e = 0; e < a.T_max * m; ++e) all = all && fin(U[e]);
  if (!all) {
    for (int k = 0; k < a.T_max; ++k) J[k] = INFINITY;
    a.T_bar[b] = a.T_min;
    return;
  }
  double running = 0.0, best = INFINITY;
  int bt = a.T_min;
  bool best_nan = false;
  for (int k = 1; k <= a.T_max; ++k) {
    double x[n], u[m];
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = X[(k - 1) * n + i];
#pragma unroll
    for (int i = 0; i < m; ++i) u[i] = U[(k - 1) * m + i];
    fwd::stage_inc<n, m>(a.c, b, x, u, running);
    if (k < a.T_min) {
      J[k - 1] = INFINITY;
      continue;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = X[k * n + i];
    bool ok = true;
    const double v = running + fwd::terminal_cost<n>(a.c, b, x, ok);
    J[k - 1] = v;
    // np.argmin: the first minimum; a NaN counts as the minimum
    if (!best_nan && (v < best || v != v)) {
      best = v;
      bt = k;
      best_nan = v != v;
    }
  }
  a.T_bar[b] = bt;
}

// ---------------------------------------------------------------- negative-time prefix
template <int SYS>
__global__ __launch_bounds__(TPB) void extend_kernel(ExtendArgs a) {
  HOP_DYN_BEGIN  // x - damping * r as NumPy rounds it: no contraction
  constexpr int n = state_dim(SYS), m = control_dim(SYS);
  const int N = a.N, S = a.S;
  const long long nx = (long long)(N + 1) * n, nu = (long long)N * m;
  const long long ex = (long long)(S + N + 1) * n, eu = (long long)(S + N) * m;
  // the tail: the workgroup copies its problems' X, U rows with coalesced accesses
  for (int p = 0; p < TPB; ++p) {
    const long long pb = (long long)blockIdx.x * TPB + p;
    if (pb >= a.batch) break;
    const double* sX = a.X + pb * nx;
    const double* sU = a.U + pb * nu;
    double* dX = a.X_ext + pb * ex + (long long)S * n;
    double* dU = a.U_ext + pb * eu + (long long)S * m;
    for (long long e = threadIdx.x; e < nx; e += TPB) dX[e] = sX[e];
    for (long long e = threadIdx.x; e < nu; e += TPB) dU[e] = sU[e];
  }
  const long long b = (long long)blockIdx.x * TPB + threadIdx.x;
  if (b >= a.batch) return;
  double* Xe = a.X_ext + b * ex;
  double* Ue = a.U_ext + b * eu;
  double u[m], xc[n];
#pragma unroll
  for (int i = 0; i < m; ++i) u[i] = a.u_fill[b * m + i];
#pragma unroll
  for (int i = 0; i < n; ++i) xc[i] = a.X[b * nx + i];
  for (int s = 1; s <= S; ++s) {
    // fixedpoint_preimage_step(F, x_next = xc, u)
    double x[n];
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = xc[i];
    for (int it = 0; it < a.max_iter; ++it) {
      double fx[n];
      eval<SYS>(x, u, a.dt, fx);
      bool f = true;
#pragma unroll
      for (int i = 0; i < n; ++i) f = f && fin(fx[i]);
      if (!f) break;
      double r[n], ss = 0.0;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        r[i] = fx[i] - xc[i];
        ss += r[i] * r[i];
      }
      if (sqrt(ss) < a.tol) break;
#pragma unroll
      for (int i = 0; i < n; ++i) x[i] = x[i] - a.damping * r[i];
    }
    bool f = true;
#pragma unroll
    for (int i = 0; i < n; ++i) f = f && fin(x[i]);
#pragma unroll
    for (int i = 0; i < n; ++i) {
      xc[i] = f ? x[i] : xc[i];  // linearization.py:162-164: keep constant
      Xe[(long long)(S - s) * n + i] = xc[i];
    }
#pragma unroll
    for (int i = 0; i < m; ++i) Ue[(long long)(S - s) * m + i] = u[i];
  }
}

// ---------------------------------------------------------------- window pick
template <int n>
__global__ __launch_bounds__(TPB) void pick_kernel(PickArgs a) {
  const long long b = (long long)blockIdx.x * TPB + threadIdx.x;
  if (b >= a.batch) return;
  const long long L = a.d.n_ext;
  a.T_star[b] = pick_one<n>(a.d, a.Vxx + b * L * n * n, a.Vx + b * L * n, a.V0 + b * L,
                            a.X_ext + b * L * n, a.x0 + b * n, a.T_bar[b],
                            a.Jw + b * a.d.T_max);
}

// ---------------------------------------------------------------- rollout
// a problem whose indices stay inside the arrays (hop_onepass.h)
__device__ inline bool roll_active(const RollArgs& a, long long b) {
  const int Ts = a.T_star[b], Tb = a.T_bar[b];
  return (a.active == nullptr || a.active[b] != 0) && Ts >= 0 && Ts <= a.N && Tb >= 0 &&
         Tb <= a.N && Ts <= Tb + a.S;
}

// pass 1: lane q = b * n_alpha + slot rolls out step size `slot`
template <int SYS>
__global__ __launch_bounds__(TPB) void rollout_kernel(RollArgs a) {
  constexpr int n = state_dim(SYS), m = control_dim(SYS);
  const long long q = (long long)blockIdx.x * TPB + threadIdx.x;
  if (q >= a.batch * a.n_alpha) return;
  const long long b = q / a.n_alpha;
  const int slot = (int)(q - b * a.n_alpha);
  double* J = a.Jc + q;
  if (!roll_active(a, b)) {
    *J = NAN;
    return;
  }
  const int N = a.N, off = a.S;
  const int T = a.T_star[b], t0 = a.T_bar[b] - T;
  const double* Xe = a.X_ext + b * (long long)(off + N + 1) * n;
  const double* Ue = a.U_ext + b * (long long)(off + N) * m;
  const double* K = a.K + b * (long long)(off + N) * m * n;
  const double* kf = a.kff + b * (long long)(off + N) * m;
  const double alpha = a.alphas[slot];
  const long long row = (long long)(N + 1) * n + (long long)N * m;
  double* Xc = a.ws + q * row;
  double* Uc = Xc + (long long)(N + 1) * n;
  double x[n];
#pragma unroll
  for (int i = 0; i < n; ++i) Xc[i] = x[i] = Xe[(long long)off * n + i];
  double acc = 0.0;
  bool ok = true;  // finite e / du along the horizon
  for (int t = 0; t < N; ++t) {
    double u[m], xn[n];
    if (t < T) {
      const long long idx = t0 + t + off;  // in [0, off + N): roll_active
      double xr[n], dx[n];
#pragma unroll
      for (int i = 0; i < n; ++i) xr[i] = Xe[idx * n + i];
      fwd::wrap_err<n>(x, xr, a.c.wrap_mask, dx);
      // u_t = U_ext[idx] + (K[idx] dx + alpha k[idx])   (solver.py:417-419)
#pragma unroll
      for (int i = 0; i < m; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < n; ++j) r = fma(K[(idx * m + i) * n + j], dx[j], r);
        u[i] = Ue[idx * m + i] + (r + alpha * kf[idx * m + i]);
      }
      ok = fwd::stage_inc<n, m>(a.c, b, x, u, acc) && ok;
    } else {
#pragma unroll
      for (int i = 0; i < m; ++i) u[i] = Ue[(long long)(off + t) * m + i];  // unshifted
    }
#pragma unroll
    for (int i = 0; i < m; ++i) Uc[t * m + i] = u[i];
    eval<SYS, true>(x, u, a.dt, xn);
    bool f = true;
#pragma unroll
    for (int i = 0; i < n; ++i) f = f && fin(xn[i]);
    if (!f) {  // a dropped step size (solver.py:421-425, 429-433)
      *J = NAN;
      return;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) Xc[(t + 1) * n + i] = x[i] = xn[i];
    if (t + 1 == T) acc += fwd::terminal_cost<n>(a.c, b, x, ok);
  }
  if (T == 0) ok = false;  // cost_timeopt_true: T* <= 0 -> inf
  *J = ok ? acc : INFINITY;
}

// pass 2: one workgroup per problem: the smallest J (strict <, alpha order), then the copy
template <int SYS>
__global__ __launch_bounds__(256) void rollout_pick_kernel(RollArgs a) {
  constexpr int n = state_dim(SYS), m = control_dim(SYS);
  const long long b = blockIdx.x;
  __shared__ int s_win;
  const int N = a.N;
  if (threadIdx.x == 0) {
    double best = INFINITY;
    int win = -1;
    for (int s = 0; s < a.n_alpha; ++s) {
      const double Jn = a.Jc[b * a.n_alpha + s];
      if (Jn < best) {  // NaN (dropped / inactive) and +inf never win
        best = Jn;
        win = s;
      }
    }
    a.accepted[b] = roll_active(a, b) ? win : -2;
    a.J[b] = best;
    s_win = win;
  }
  __syncthreads();
  const int win = s_win;
  const long long nx = (long long)(N + 1) * n, nu = (long long)N * m;
  const double* srcX = win >= 0 ? a.ws + (b * a.n_alpha + win) * (nx + nu)
                                : a.X_ext + (b * (long long)(a.S + N + 1) + a.S) * n;
  const double* srcU = win >= 0 ? srcX + nx : a.U_ext + (b * (long long)(a.S + N) + a.S) * m;
  double* dX = a.X_new + b * nx;
  double* dU = a.U_new + b * nu;
  for (long long e = threadIdx.x; e < nx; e += 256) dX[e] = srcX[e];
  for (long long e = threadIdx.x; e < nu; e += 256) dU[e] = srcU[e];
}

template <int SYS>
hipError_t launch(int which, const void* args, hipStream_t st) {
  switch (which) {
    case 0: {
      const CurveArgs& a = *(const CurveArgs*)args;
      hipLaunchKernelGGL((curve_kernel<SYS>), dim3((unsigned)((a.batch + TPB - 1) / TPB)),
                         dim3(TPB), 0, st, a);
      break;
    }
    case 1: {
      const ExtendArgs& a = *(const ExtendArgs*)args;
      hipLaunchKernelGGL((extend_kernel<SYS>), dim3((unsigned)((a.batch + TPB - 1) / TPB)),
                         dim3(TPB), 0, st, a);
      break;
    }
    default: {
      const RollArgs& a = *(const RollArgs*)args;
      const long long lanes = a.batch * a.n_alpha;
      hipLaunchKernelGGL((rollout_kernel<SYS>), dim3((unsigned)((lanes + TPB - 1) / TPB)),
                         dim3(TPB), 0, st, a);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((rollout_pick_kernel<SYS>), dim3((unsigned)a.batch), dim3(256), 0, st,
                         a);
    }
  }
  return hipGetLastError();
}

hipError_t dispatch(int sys, int which, const void* args, hipStream_t stream) {
  switch (sys) {
    case kDI: return launch<kDI>(which, args, stream);
    case kCartpole: return launch<kCartpole>(which, args, stream);
    case kQuadrotor: return launch<kQuadrotor>(which, args, stream);
    case kPointmass: return launch<kPointmass>(which, args, stream);
    default: return launch<kSegway>(which, args, stream);
  }
}

hipError_t dispatch_pick(const PickArgs& a, int n, hipStream_t st) {
  const dim3 grid((unsigned)((a.batch + TPB - 1) / TPB));
  switch (n) {
    case 2: hipLaunchKernelGGL((pick_kernel<2>), grid, dim3(TPB), 0, st, a); break;
    case 4: hipLaunchKernelGGL((pick_kernel<4>), grid, dim3(TPB), 0, st, a); break;
    default: hipLaunchKernelGGL((pick_kernel<12>), grid, dim3(TPB), 0, st, a);
  }
  return hipGetLastError();
}

// hop_cost_true_f64's checks of the cost arguments (an empty batch needs no pointers)
int cost_args(bool empty, int32_t system, const double* xg, int64_t xg_bs, const double* u_ref,
              int64_t ur_bs, const double* Q, int64_t q_bs, const double* R, int64_t r_bs,
              const double* Qf, int64_t qf_bs, const double* w, int64_t w_bs,
              const double* obstacles, int32_t n_obs, uint32_t wrap_mask, CostArgs* c) {
  if (system < 0 || system >= kNumSystems) return set_error(HOP_E_ARG, "unknown system id");
  if (!empty && (!xg || !u_ref || !Q || !R || !Qf || !w))
    return set_error(HOP_E_ARG, "null cost parameter");
  if (xg_bs < 0 || ur_bs < 0 || q_bs < 0 || r_bs < 0 || qf_bs < 0 || w_bs < 0)
    return set_error(HOP_E_ARG, "negative batch stride");
  if (n_obs < 0 || n_obs > 64 || (!empty && n_obs > 0 && !obstacles))
    return set_error(HOP_E_ARG, "obstacles: 0 <= n_obs <= 64 rows of (cx, cy, radius, weight)");
  const int n = state_dim(system);
  if (n_obs > 0 && n < 2) return set_error(HOP_E_ARG, "obstacles need a planar position (n >= 2)");
  if (wrap_mask >> n) return set_error(HOP_E_ARG, "wrap index out of range");
  *c = CostArgs{xg, xg_bs, u_ref, ur_bs, Q, q_bs, R, r_bs, Qf, qf_bs, w, w_bs,
                n_obs > 0 ? obstacles : nullptr, n_obs, wrap_mask};
  return HOP_OK;
}

constexpr int64_t kMaxLanes = (int64_t)0x7fffffffLL * TPB;  // one launch's grid

}  // namespace onepass
}  // namespace hop

using hop::set_error;
using hop::set_hip_status;
namespace op = hop::onepass;

extern "C" {

int hop_onepass_nominal_curve_f64(int32_t system, const double* X, const double* U,
                                  const double* xg, int64_t xg_bs, const double* u_ref,
                                  int64_t ur_bs, const double* Q, int64_t q_bs, const double* R,
                                  int64_t r_bs, const double* Qf, int64_t qf_bs, const double* w,
                                  int64_t w_bs, const double* obstacles, int32_t n_obs,
                                  uint32_t wrap_mask, int32_t T_min, int32_t T_max, int64_t batch,
                                  int32_t N, double* J, int32_t* T_bar, void* stream) {
  op::CurveArgs a{};
  int rc = op::cost_args(batch == 0, system, xg, xg_bs, u_ref, ur_bs, Q, q_bs, R, r_bs, Qf, qf_bs, w, w_bs,
                         obstacles, n_obs, wrap_mask, &a.c);
  if (rc) return rc;
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if (T_min < 1 || T_max < T_min || T_max > N)
    return set_error(HOP_E_ARG, "need 1 <= T_min <= T_max <= N");
  if (batch == 0) return HOP_OK;
  if (!X || !U || !J || !T_bar) return set_error(HOP_E_ARG, "null pointer");
  if (batch > op::kMaxLanes) return set_error(HOP_E_SIZE, "batch too large for one launch");
  a.X = X; a.U = U; a.batch = batch; a.N = N; a.T_min = T_min; a.T_max = T_max;
  a.J = J; a.T_bar = T_bar;
  return set_hip_status(op::dispatch(system, 0, &a, (hipStream_t)stream));
}

int hop_onepass_extend_backward_f64(int32_t system, double dt, const double* X, const double* U,
                                    const double* u_fill, int64_t batch, int32_t N, int32_t S,
                                    int32_t max_iter, double tol, double damping, double* X_ext,
                                    double* U_ext, void* stream) {
  if (system < 0 || system >= hop::dyn::kNumSystems)
    return set_error(HOP_E_ARG, "unknown system id");
  if (batch < 0 || N < 0 || max_iter < 0) return set_error(HOP_E_ARG, "negative size");
  if (S < 1) return set_error(HOP_E_ARG, "the prefix needs S >= 1");
  if (S > HOP_ONEPASS_MAX_WINDOW) return set_error(HOP_E_SIZE, "S above HOP_ONEPASS_MAX_WINDOW");
  if (batch == 0) return HOP_OK;
  if (!X || !u_fill || !X_ext || !U_ext || (N > 0 && !U))
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > op::kMaxLanes) return set_error(HOP_E_SIZE, "batch too large for one launch");
  op::ExtendArgs a{dt, X, U, u_fill, batch, N, S, max_iter, tol, damping, X_ext, U_ext};
  return set_hip_status(op::dispatch(system, 1, &a, (hipStream_t)stream));
}

int hop_onepass_pick_f64(const double* Vxx, const double* Vx, const double* V0,
                         const double* X_ext, const double* x0, const int32_t* T_bar,
                         int64_t batch, int32_t n, int32_t n_ext, int32_t T_min, int32_t T_max,
                         int32_t S_left, int32_t S_right, uint32_t wrap_mask,
                         double locality_mult, int32_t* T_star, double* Jw, void* stream) {
  if (n != 2 && n != 4 && n != 12)
    return set_error(HOP_E_SIZE, "n must be a built-in system's state size (2, 4, 12)");
  if (batch < 0 || n_ext < 1) return set_error(HOP_E_ARG, "negative size");
  if (T_min < 1 || T_max < T_min) return set_error(HOP_E_ARG, "need 1 <= T_min <= T_max");
  if (S_left < 0 || S_right < 0) return set_error(HOP_E_ARG, "negative window");
  if (S_left > HOP_ONEPASS_MAX_WINDOW || S_right > HOP_ONEPASS_MAX_WINDOW)
    return set_error(HOP_E_SIZE, "window above HOP_ONEPASS_MAX_WINDOW");
  if (wrap_mask >> n) return set_error(HOP_E_ARG, "wrap index out of range");
  if (batch == 0) return HOP_OK;
  if (!Vxx || !Vx || !V0 || !X_ext || !x0 || !T_bar || !T_star || !Jw)
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > op::kMaxLanes) return set_error(HOP_E_SIZE, "batch too large for one launch");
  op::PickArgs a{{n_ext, T_min, T_max, S_left, S_right, wrap_mask, locality_mult},
                 Vxx, Vx, V0, X_ext, x0, T_bar, batch, T_star, Jw};
  return set_hip_status(op::dispatch_pick(a, n, (hipStream_t)stream));
}

size_t hop_onepass_rollout_workspace_bytes(int32_t system, int64_t batch, int32_t N,
                                           int32_t n_alpha) {
  if (system < 0 || system >= hop::dyn::kNumSystems || batch < 0 || N < 0 || n_alpha < 0)
    return 0;
  const int64_t n = hop::dyn::state_dim(system), m = hop::dyn::control_dim(system);
  const int64_t row = (int64_t)(N + 1) * n + (int64_t)N * m;
  return (size_t)(batch * n_alpha * (1 + row) * (int64_t)sizeof(double));
}

int hop_onepass_rollout_f64(int32_t system, double dt, const double* X_ext, const double* U_ext,
                            const double* xg, int64_t xg_bs, const double* u_ref, int64_t ur_bs,
                            const double* Q, int64_t q_bs, const double* R, int64_t r_bs,
                            const double* Qf, int64_t qf_bs, const double* w, int64_t w_bs,
                            const double* obstacles, int32_t n_obs, uint32_t wrap_mask,
                            const int32_t* T_bar, const int32_t* T_star, const int32_t* active,
                            const double* K, const double* k, const double* alphas,
                            int32_t n_alpha, int64_t batch, int32_t N, int32_t S, void* workspace,
                            size_t workspace_bytes, double* X_new, double* U_new, double* J,
                            int32_t* accepted, void* stream) {
  op::RollArgs a{};
  int rc = op::cost_args(batch == 0, system, xg, xg_bs, u_ref, ur_bs, Q, q_bs, R, r_bs, Qf, qf_bs, w, w_bs,
                         obstacles, n_obs, wrap_mask, &a.c);
  if (rc) return rc;
  if (batch < 0 || N < 0 || S < 0) return set_error(HOP_E_ARG, "negative size");
  if (S > HOP_ONEPASS_MAX_WINDOW) return set_error(HOP_E_SIZE, "S above HOP_ONEPASS_MAX_WINDOW");
  if (n_alpha < 1 || n_alpha > 8 || !alphas)
    return set_error(HOP_E_ARG, "1 <= n_alpha <= 8 host alphas");
  if (batch == 0) return HOP_OK;
  if (!X_ext || !T_bar || !T_star || !X_new || !U_new || !J || !accepted ||
      (S + N > 0 && (!U_ext || !K || !k)))
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > 0x7fffffffLL) return set_error(HOP_E_SIZE, "batch too large for one launch");
  const size_t need = hop_onepass_rollout_workspace_bytes(system, batch, N, n_alpha);
  if (!workspace || workspace_bytes < need) return set_error(HOP_E_ARG, "workspace too small");
  a.dt = dt; a.X_ext = X_ext; a.U_ext = U_ext; a.T_bar = T_bar; a.T_star = T_star;
  a.active = active; a.K = K; a.kff = k;
  for (int i = 0; i < n_alpha; ++i) a.alphas[i] = alphas[i];
  a.n_alpha = n_alpha; a.batch = batch; a.N = N; a.S = S;
  a.Jc = (double*)workspace;
  a.ws = a.Jc + batch * n_alpha;
  a.X_new = X_new; a.U_new = U_new; a.J = J; a.accepted = accepted;
  return set_hip_status(op::dispatch(system, 2, &a, (hipStream_t)stream));
}

}  // extern "C"
