// The row-per-trajectory skeleton of the wide device systems (chain.hip, fleet.hip):
// one trajectory per 16-lane DPP row, four per wave64, 16 per 256-thread workgroup.
// Everything the systems share -- the call structs, the control flow of the rollout, the
// true cost and the line search (solver.py:42-102, 233-286), the C entries' argument
// checks -- is written once over a row policy `Sys`, which supplies what differs:
//   Par, n(P), m(P)       the parameter block, the stacked sizes (host and device)
//   Lane, lane_of(P)      what a lane is within its row
//   State, Input          a lane's share of x and u: load_x / store_x / nan_x, load_u /
//                         store_u, nonfinite(x), norm2(x) = the lane's share of |x|^2
//   step(P, l, x, u)      one step of the row
//   Lds, stage(c, P, lds) the workgroup's LDS (one __shared__ struct per kernel), staged
//                         by all 256 threads; returns whether the blocks allow the
//                         system's fast path (the chain: all diagonal)
//   RowCost, row_cost_of  what a row needs of the cost
//   stage_inc, terminal_cost   acc += (0.5 e.Qe + 0.5 du.R du) + w and 0.5 e.Qf e in the
//                         reference's order; a non-finite e or du clears `ok` by row_any
//   feedback              U'[k] = U[k] + (K_k dx + alpha k_k) on the lane's inputs
// Every policy function is __device__ __forceinline__ (HOP_ROWFN): no virtual calls, no
// function pointers.  Every decision a whole row takes (stop, reject) goes through
// row_any here, so the lanes of a row never part.  The J_old rows and the candidate rows
// of the line search run the same stage function.
#pragma once
#include <math.h>

#include "hop_device.hpp"
#include "hop_kernels.hpp"

#define HOP_ROWFN static __device__ __forceinline__

namespace hop {
namespace rowsys {

constexpr int TPB = 256;                 // 16 rows per workgroup
constexpr int kRows = TPB / kRowLanes;
inline unsigned row_grid(long long rows) { return (unsigned)((rows + kRows - 1) / kRows); }
// one launch holds at most 2^32 work-items: rows of 16 lanes, whole workgroups
constexpr int64_t kMaxItems = 0xffffffffLL;
constexpr int64_t kMaxRows = kMaxItems / kRowLanes - kRows;
inline bool rows_fit(int64_t rows) { return rows <= kMaxRows; }

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }
__device__ __forceinline__ int row_lane() { return threadIdx.x & 15; }
// the global index of this lane's row
__device__ __forceinline__ long long row_index() {
  return (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
}
// true on every lane of a row when pred holds on any of its lanes
__device__ __forceinline__ bool row_any(bool pred) {
  const unsigned long long b = __ballot(pred);
  return ((b >> (threadIdx.x & 48)) & 0xffffull) != 0ull;
}

struct CostC {
  const double* xg; long long xg_bs;     // [B or 1][n]
  const double* u_ref; long long ur_bs;  // [B or 1][m]
  const double* Q; const double* R; const double* Qf;  // shared
  const double* w; long long w_bs;       // [B or 1]
  unsigned wrap_mask;                    // the chain wraps nothing: 0
};
template <class Par>
struct DynC {
  Par P;
  const double* X; const double* U; double* Xn;
  long long count, x_stride, u_stride, xn_stride;
};
template <class Par>
struct RolloutC {
  Par P;
  const double* x0; long long x0_bs;
  const double* U; long long batch; int N;
  double max_state_norm;
  double* X;
};
template <class Par>
struct CostCallC {
  Par P;
  CostC c;
  const double* X; const double* U; const int* T;
  long long batch; int N;
  double* J;
};
template <class Par>
struct FwdC {
  Par P;
  CostC c;
  const double* X; const double* U;
  const int* T_star; const int* active;
  const double* K; const double* kff;
  double alphas[8]; int n_alpha;
  long long batch; int N;
  double* Jc;     // workspace [B][n_alpha]
  double* ws;     // workspace [B][n_alpha][(N+1) n + N m]
  double* J_old;
  double* X_new; double* U_new; double* J; int* accepted;
};
template <class Par>
struct LinC {
  Par P;
  int central;
  double epsx, epsu, relx, relu;
  const double* X; const double* U;
  long long batch; int nalloc, nuse;
  double* A; double* B; double* a_res; double* Fx;
};

// cost_timeopt_true of one row's X [N+1][n], U [N][m] at horizon T (T <= N)
template <class Sys>
__device__ double row_cost_true(const typename Sys::RowCost& rc, const typename Sys::Par& P,
                                const typename Sys::Lane& l, const double* X, const double* U,
                                int T) {
  if (T <= 0) return INFINITY;
  const int n = Sys::n(P), m = Sys::m(P);
  double acc = 0.0;
  bool ok = true;
  for (int k = 0; k < T; ++k)
    ok = Sys::stage_inc(rc, l, Sys::load_x(X + (long long)k * n, P, l),
                        Sys::load_u(U + (long long)k * m, P, l), acc) && ok;
  const double t = Sys::terminal_cost(rc, l, Sys::load_x(X + (long long)T * n, P, l), ok);
  return ok ? acc + t : INFINITY;
}

// ---------------------------------------------------------------- single step
template <class Sys>
__global__ __launch_bounds__(TPB) void dynamics_kernel(DynC<typename Sys::Par> a) {
  const long long r = row_index();
  if (r >= a.count) return;
  const typename Sys::Par P = a.P;
  const auto l = Sys::lane_of(P);
  const auto x = Sys::load_x(a.X + r * a.x_stride, P, l);
  const auto u = Sys::load_u(a.U + r * a.u_stride, P, l);
  Sys::store_x(a.Xn + r * a.xn_stride, P, l, Sys::step(P, l, x, u));
}

// ---------------------------------------------------------------- rollout
template <class Sys>
__global__ __launch_bounds__(TPB) void rollout_kernel(RolloutC<typename Sys::Par> a) {
  const long long b = row_index();
  if (b >= a.batch) return;
  const typename Sys::Par P = a.P;
  const auto l = Sys::lane_of(P);
  const int n = Sys::n(P), m = Sys::m(P), N = a.N;
  const double* U = a.U + b * (long long)N * m;
  double* X = a.X + b * (long long)(N + 1) * n;
  auto x = Sys::load_x(a.x0 + b * a.x0_bs, P, l);
  Sys::store_x(X, P, l, x);
  int k = 0;
  for (; k < N; ++k) {
    const auto xn = Sys::step(P, l, x, Sys::load_u(U + (long long)k * m, P, l));
    const double ss = lane_sum<16>(Sys::norm2(xn));
    // reference: not finite or np.linalg.norm(xn) > max_state_norm -> X[k+1:] = NaN, on
    // the whole state (lane_sum leaves the same bits on every lane, so any lane = all)
    if (row_any(Sys::nonfinite(xn) || sqrt(ss) > a.max_state_norm)) break;
    x = xn;
    Sys::store_x(X + (long long)(k + 1) * n, P, l, x);
  }
  const auto nan = Sys::nan_x();
  for (int r = k + 1; r <= N; ++r) Sys::store_x(X + (long long)r * n, P, l, nan);
}

// ---------------------------------------------------------------- cost
template <class Sys>
__global__ __launch_bounds__(TPB) void cost_kernel(CostCallC<typename Sys::Par> a) {
  __shared__ typename Sys::Lds lds;
  const typename Sys::Par P = a.P;
  const bool fast = Sys::stage(a.c, P, lds);
  const long long b = row_index();
  if (b >= a.batch) return;
  const auto l = Sys::lane_of(P);
  const int n = Sys::n(P), m = Sys::m(P), N = a.N;
  const int T = a.T[b];
  double J = NAN;
  if (T <= N) {
    const auto rc = Sys::row_cost_of(a.c, P, l, b, lds, fast);
    J = row_cost_true<Sys>(rc, P, l, a.X + b * (long long)(N + 1) * n, a.U + b * (long long)N * m,
                           T);
  }
  if (row_lane() == 0) a.J[b] = J;
}

// ---------------------------------------------------------------- line search
// pass 1: row b * n_alpha + slot rolls out step size `slot` of problem b; the rows
// after them, one per problem, compute J_old.  Pass 2 is forward.hip's pick kernel.
template <class Sys>
__global__ __launch_bounds__(TPB) void linesearch_kernel(FwdC<typename Sys::Par> a) {
  __shared__ typename Sys::Lds lds;
  const typename Sys::Par P = a.P;
  const bool fast = Sys::stage(a.c, P, lds);
  const long long rg = row_index();
  const long long nr = a.batch * a.n_alpha;
  if (rg >= nr + a.batch) return;
  const auto l = Sys::lane_of(P);
  const int n = Sys::n(P), m = Sys::m(P), N = a.N;
  const bool roll = rg < nr;
  const long long b = roll ? rg / a.n_alpha : rg - nr;
  const int slot = roll ? (int)(rg - b * a.n_alpha) : a.n_alpha;
  const double* X = a.X + b * (long long)(N + 1) * n;
  const double* U = a.U + b * (long long)N * m;
  const int T = a.T_star[b];
  const auto rc = Sys::row_cost_of(a.c, P, l, b, lds, fast);
  if (!roll) {
    const double Jo = T > N ? NAN : row_cost_true<Sys>(rc, P, l, X, U, T);
    if (row_lane() == 0) a.J_old[b] = Jo;
    return;
  }
  const bool active = (a.active == nullptr || a.active[b] != 0) && T >= 0 && T <= N;
  double* J = a.Jc + b * a.n_alpha + slot;
  if (!active) {
    if (row_lane() == 0) *J = NAN;
    return;
  }
  const double alpha = a.alphas[slot];
  const double* K = a.K + b * (long long)N * m * n;
  const double* kf = a.kff + b * (long long)N * m;
  const long long row = (long long)(N + 1) * n + (long long)N * m;
  double* Xc = a.ws + (b * a.n_alpha + slot) * row;
  double* Uc = Xc + (long long)(N + 1) * n;
  auto x = Sys::load_x(X, P, l);
  Sys::store_x(Xc, P, l, x);
  double acc = 0.0;
  bool ok = true;  // finite e / du along the horizon
  for (int k = 0; k < N; ++k) {
    const double* Uk = U + (long long)k * m;
    typename Sys::Input u;
    if (k < T) {
      // U'[k] = U[k] + (K_k dx + alpha k_k)   (solver.py:262-263)
      u = Sys::feedback(rc, P, l, x, X + (long long)k * n, Uk, K + (long long)k * m * n,
                        kf + (long long)k * m, alpha);
      ok = Sys::stage_inc(rc, l, x, u, acc) && ok;
    } else {
      u = Sys::load_u(Uk, P, l);
    }
    Sys::store_u(Uc + (long long)k * m, P, l, u);
    const auto xn = Sys::step(P, l, x, u);
    if (row_any(Sys::nonfinite(xn))) {  // rejected step size (solver.py:265-267, 272-274)
      if (row_lane() == 0) *J = NAN;
      return;
    }
    x = xn;
    Sys::store_x(Xc + (long long)(k + 1) * n, P, l, x);
    if (k + 1 == T) acc += Sys::terminal_cost(rc, l, x, ok);
  }
  if (T == 0) ok = false;  // cost_timeopt_true: T* <= 0 -> inf
  if (row_lane() == 0) *J = ok ? acc : INFINITY;
}

// ---------------------------------------------------------------- C entries
// each: the system's validated Par and its entry's C arguments -> checks, struct, launch
template <class Sys>
int dynamics_entry(const typename Sys::Par& P, const double* X, int64_t x_stride, const double* U,
                   int64_t u_stride, int64_t count, double* Xn, int64_t xn_stride, void* stream) {
  if (count < 0) return set_error(HOP_E_ARG, "count < 0");
  if (count == 0) return HOP_OK;
  if (!X || !U || !Xn) return set_error(HOP_E_ARG, "null input/output pointer");
  if (x_stride < Sys::n(P) || u_stride < Sys::m(P) || xn_stride < Sys::n(P))
    return set_error(HOP_E_ARG, "row stride too small");
  if (!rows_fit(count)) return set_error(HOP_E_SIZE, "count too large for one launch");
  const DynC<typename Sys::Par> a{P, X, U, Xn, count, x_stride, u_stride, xn_stride};
  hipLaunchKernelGGL(dynamics_kernel<Sys>, dim3(row_grid(count)), dim3(TPB), 0,
                     (hipStream_t)stream, a);
  return set_hip_status(hipGetLastError());
}

template <class Sys>
int rollout_entry(const typename Sys::Par& P, const double* x0, int64_t x0_batch_stride,
                  const double* U, int64_t batch, int32_t N, double max_state_norm, double* X,
                  void* stream) {
  if (batch < 0 || N < 0 || x0_batch_stride < 0)
    return set_error(HOP_E_ARG, "negative size/stride");
  if (batch == 0) return HOP_OK;
  if (!x0 || !X || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  const RolloutC<typename Sys::Par> a{P, x0, x0_batch_stride, U, batch, N, max_state_norm, X};
  hipLaunchKernelGGL(rollout_kernel<Sys>, dim3(row_grid(batch)), dim3(TPB), 0,
                     (hipStream_t)stream, a);
  return set_hip_status(hipGetLastError());
}

// The checks of both linearise entries; max_units bounds batch * n_use, the waves or rows
// of the system's own launch.  kNothing: a valid call with no step to linearise (the
// entry returns HOP_OK); an error code is negative.
constexpr int kNothing = 1;
inline int linearize_checks(const double* X, const double* U, int64_t batch, int32_t n_alloc,
                            int32_t n_use, int32_t central, const double* A, const double* Bm,
                            int64_t max_units) {
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n_alloc < 0) return set_error(HOP_E_ARG, "n_alloc < 0");
  if (n_use > n_alloc) return set_error(HOP_E_ARG, "n_use > n_alloc");
  if (central != 0 && central != 1) return set_error(HOP_E_ARG, "central must be 0 or 1");
  if (batch == 0 || n_use <= 0) return kNothing;
  if (!X || !U || !A || !Bm) return set_error(HOP_E_ARG, "null input/output pointer");
  if (batch > kMaxItems || batch * (int64_t)n_use > max_units)
    return set_error(HOP_E_SIZE, "batch * n_use too large for one launch");
  return HOP_OK;
}

// the cost arguments of the true-cost and line-search entries, as the entry packed them
inline int cost_check(const CostC& c) {
  if (!c.xg || !c.u_ref || !c.Q || !c.R || !c.Qf || !c.w)
    return set_error(HOP_E_ARG, "null cost parameter");
  if (c.xg_bs < 0 || c.ur_bs < 0 || c.w_bs < 0)
    return set_error(HOP_E_ARG, "negative batch stride");
  return HOP_OK;
}

template <class Sys>
int cost_entry(const typename Sys::Par& P, const double* X, const double* U, const int32_t* T_star,
               const CostC& cost, int64_t batch, int32_t N, double* J, void* stream) {
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if ((uint64_t)cost.wrap_mask >> Sys::n(P)) return set_error(HOP_E_ARG, "wrap bits at or above n");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_check(cost)) return rc;
  if (!X || !T_star || !J || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  const CostCallC<typename Sys::Par> a{P, cost, X, U, T_star, batch, N, J};
  hipLaunchKernelGGL(cost_kernel<Sys>, dim3(row_grid(batch)), dim3(TPB), 0, (hipStream_t)stream,
                     a);
  return set_hip_status(hipGetLastError());
}

// the line search's workspace: J' and [X' | U'] per (problem, step size)
inline size_t workspace_bytes(int64_t n, int64_t m, int64_t batch, int32_t N, int32_t n_alpha) {
  if (batch < 0 || N < 0 || n_alpha < 0) return 0;
  const int64_t row = (int64_t)(N + 1) * n + (int64_t)N * m;
  return (size_t)(batch * n_alpha * (1 + row) * (int64_t)sizeof(double));
}

template <class Sys>
int linesearch_entry(const typename Sys::Par& P, const double* X, const double* U,
                     const CostC& cost, const int32_t* T_star, const int32_t* active,
                     const double* K, const double* k, const double* alphas, int32_t n_alpha,
                     int64_t batch, int32_t N, void* workspace, size_t workspace_bytes_given,
                     double* X_new, double* U_new, double* J, double* J_old, int32_t* accepted,
                     void* stream) {
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if (n_alpha < 1 || n_alpha > 8 || !alphas)
    return set_error(HOP_E_ARG, "1 <= n_alpha <= 8 host alphas");
  if ((uint64_t)cost.wrap_mask >> Sys::n(P)) return set_error(HOP_E_ARG, "wrap bits at or above n");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_check(cost)) return rc;
  if (!X || !T_star || !K || !k || !X_new || !U_new || !J || !J_old || !accepted ||
      (N > 0 && !U))
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > kMaxItems / TPB || !rows_fit(batch * (n_alpha + 1)))
    return set_error(HOP_E_SIZE, "batch too large for one launch");
  const size_t need = workspace_bytes(Sys::n(P), Sys::m(P), batch, N, n_alpha);
  if (!workspace || workspace_bytes_given < need)
    return set_error(HOP_E_ARG, "workspace too small");
  double* Jc = (double*)workspace;
  FwdC<typename Sys::Par> a{P, cost, X, U, T_star, active, K, k, {}, n_alpha, batch, N, Jc,
                            Jc + batch * n_alpha, J_old, X_new, U_new, J, accepted};
  for (int i = 0; i < n_alpha; ++i) a.alphas[i] = alphas[i];
  hipLaunchKernelGGL(linesearch_kernel<Sys>, dim3(row_grid(batch * (n_alpha + 1))), dim3(TPB), 0,
                     (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_hip_status(e);
  return set_hip_status(launch_linesearch_pick(pick_args_of(a, Sys::n(P), Sys::m(P)),
                                               (hipStream_t)stream));
}

}  // namespace rowsys
}  // namespace hop
