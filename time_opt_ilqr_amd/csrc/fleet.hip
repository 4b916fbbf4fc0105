// Fleets of the built-in systems as device systems (include/hop_fleet.h): `count`
// copies of one system of dynamics.hpp, stacked member-major and coupled only through
// the dense cost blocks, so that a joint solve's rollout, true cost, forward line search
// and FD linearisation run without the host.
//   rollout                    solver.py:42-62            hop_fleet_rollout_f64
//   cost_timeopt_true          solver.py:65-102           hop_fleet_cost_true_f64
//   forward_linesearch_fixedT  solver.py:233-286          hop_fleet_forward_linesearch_f64
//   linearize_*_diff_traj, compute_affine_residuals
//                              linearization.py:177-270   hop_fleet_linearize_f64
// The member system is a template constant (its state stays in registers indexed by
// unrolled constants); the member count is a run-time argument.
//
// Row layout (everything sequential in time): one trajectory -- or one (problem, step)
// pair of the linearisation -- per 16-lane DPP row, four per wave64.  Lane a holds member
// a: its n_s states and m_s inputs, the matching entries of xg, u_ref, e, du and dx, and
// its bits of the wrap mask; lanes >= count hold exact zeros and evaluate nothing.  A
// member steps by dyn::eval<SYS> on its own lane, so a fleet step is bit for bit the
// members' steps.  What crosses members goes through LDS: the dense Q, Qf and R of the
// workgroup, and one 32-entry vector per row into which the lanes write their slices of
// e, du or dx; lane a then forms its own rows of Q e, R du or K_k dx from the whole
// vector (one ascending fma chain per row) and the row sums v.(M v) and the squared
// state norm with the DPP butterfly of hop_device.hpp.  A decision a whole row takes
// (stop, reject) comes from a ballot, never from a lane's own copy of a row sum.  The
// per-step accumulation c += (0.5 e.Qe + 0.5 du.R du) + w and the terminal term keep the
// reference's order; the J_old rows and the candidate rows run the same stage function.
//
// Linearisation: lane a evaluates member a's base point and finite-difference columns
// (fleet_math.hpp, linearize.hip's arithmetic) and writes rows [a n_s, (a + 1) n_s) of
// A_k and B_k in full, the off-block entries by the reference's rule.
#include <math.h>

#include "hop_device.hpp"
#include "hop_kernels.hpp"
#include "fleet_math.hpp"
#include "../../include/hop_fleet.h"

namespace hop {
namespace fleet {

constexpr int TPB = 256;                 // 16 rows per workgroup
constexpr int kRows = TPB / kRowLanes;
constexpr int kVec = 32;                 // a row's exchange vector: n <= 31, m <= 16
constexpr int kCostLds = 2 * kMaxN * kMaxN + kMaxM * kMaxM;  // Q, Qf, R (dense, packed)

struct Par {
  int sys, count;
  double dt;
};
struct CostC {
  const double* xg; long long xg_bs;     // [B or 1][n]
  const double* u_ref; long long ur_bs;  // [B or 1][m]
  const double* Q; const double* R; const double* Qf;  // shared
  const double* w; long long w_bs;       // [B or 1]
  unsigned wrap_mask;
};
struct DynC {
  Par P;
  const double* X; const double* U; double* Xn;
  long long count, x_stride, u_stride, xn_stride;
};
struct RolloutC {
  Par P;
  const double* x0; long long x0_bs;
  const double* U; long long batch; int N;
  double max_state_norm;
  double* X;
};
struct CostCallC {
  Par P;
  CostC c;
  const double* X; const double* U; const int* T;
  long long batch; int N;
  double* J;
};
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
struct LinC {
  Par P;
  int central;
  double epsx, epsu, relx, relu;
  const double* X; const double* U;
  long long batch; int nalloc, nuse;
  double* A; double* B; double* a_res; double* Fx;
};

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }

// true on every lane of a row when pred holds on any of its lanes / on its first lane
__device__ __forceinline__ bool row_any(bool pred) {
  const unsigned long long b = __ballot(pred);
  return ((b >> (threadIdx.x & 48)) & 0xffffull) != 0ull;
}
__device__ __forceinline__ bool row_first(bool pred) {
  const unsigned long long b = __ballot(pred);
  return ((b >> (threadIdx.x & 48)) & 1ull) != 0ull;
}

// what a lane is within its row
struct Lane {
  int a;      // lane of the row = member
  bool live;  // a < count
};
__device__ __forceinline__ Lane lane_of(const Par& P) {
  Lane l;
  l.a = threadIdx.x & 15;
  l.live = l.a < P.count;
  return l;
}

template <int K>
__device__ __forceinline__ void load_slice(const double* p, const Lane& l, double (&v)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = l.live ? p[l.a * K + i] : 0.0;
}
template <int K>
__device__ __forceinline__ void store_slice(double* p, const Lane& l, const double (&v)[K]) {
  if (l.live) {
#pragma unroll
    for (int i = 0; i < K; ++i) p[l.a * K + i] = v[i];
  }
}

// One step of a row: member a on lane a; idle lanes keep zeros.  The rollout, the line
// search and the single-step kernel all step through this.
template <int SYS>
__device__ __forceinline__ void row_step(const Lane& l, const double* x, const double* u,
                                         double dt, double* xn) {
  constexpr int ns = state_dim(SYS);
#pragma unroll
  for (int i = 0; i < ns; ++i) xn[i] = 0.0;
  if (l.live) eval<SYS>(x, u, dt, xn);
}

// ---- cost blocks in LDS ------------------------------------------------------
// sc: Q [n][n], then Qf [n][n], then R [m][m], packed
__device__ __forceinline__ void stage_cost(const CostC& c, int n, int m, double* sc) {
  const int nq = n * n, tot = 2 * nq + m * m;
  for (int e = threadIdx.x; e < tot; e += TPB)
    sc[e] = e < nq ? c.Q[e] : e < 2 * nq ? c.Qf[e - nq] : c.R[e - 2 * nq];
  __syncthreads();
}

// 0.5 v.(M v) for a dense dim x dim block M in LDS, lane a holding v[a K .. a K + K):
// the lanes publish their slices in the row's vector, lane a forms rows a K .. of M v.
// Every lane of the row gets the sum (use one lane's copy only).
template <int K>
__device__ __forceinline__ double half_quad_row(const double* M, int dim, const Lane& l,
                                                const double (&v)[K], double* vec) {
  wave_sync();  // the vector's readers of the step before are done
  store_slice<K>(vec, l, v);
  wave_sync();
  double part = 0.0;
  if (l.live) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double* row = M + (l.a * K + i) * dim;
      double r = 0.0;
      for (int c = 0; c < dim; ++c) r = fma(row[c], vec[c], r);
      part = fma(v[i], r, part);
    }
  }
  return 0.5 * lane_sum<16>(part);
}

// what a row needs of the cost: its lane's entries of xg and u_ref, its wrap bits, w,
// the LDS blocks and the row's exchange vector
template <int SYS>
struct RowCost {
  static constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const double* sQ; const double* sQf; const double* sR;
  double* vec;
  int n, m;
  unsigned wm;  // bits [a n_s, (a + 1) n_s) of the wrap mask
  double xg[ns], ur[ms], w;
};
template <int SYS>
__device__ __forceinline__ RowCost<SYS> row_cost_of(const CostC& c, const Par& P, const Lane& l,
                                                    long long b, double* sc, double* vec) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  RowCost<SYS> r;
  r.n = P.count * ns, r.m = P.count * ms;
  r.sQ = sc, r.sQf = sc + r.n * r.n, r.sR = sc + 2 * r.n * r.n;
  r.vec = vec;
  r.wm = l.live ? (c.wrap_mask >> (l.a * ns)) & ((1u << ns) - 1u) : 0u;
  load_slice<ns>(c.xg + b * c.xg_bs, l, r.xg);
  load_slice<ms>(c.u_ref + b * c.ur_bs, l, r.ur);
  r.w = c.w[b * c.w_bs];
  return r;
}

// a - b on the lane's slice, wrapped where the member's mask says so (utils.py:127-137)
template <int K>
__device__ __forceinline__ void wrap_diff(const double* a, const double* b, unsigned wm,
                                          double (&e)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double d = a[i] - b[i];
    e[i] = (wm >> i) & 1u ? wrap_angle(d) : d;
  }
}

// running-cost increment of one step (solver.py:87-95): acc += (q + r) + w; returns
// false if e or du is not finite in any member
template <int SYS>
__device__ __forceinline__ bool stage_inc(const RowCost<SYS>& rc, const Lane& l, const double* x,
                                          const double* u, double& acc) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  double e[ns], du[ms];
  wrap_diff<ns>(x, rc.xg, rc.wm, e);
  bool bad = false;
#pragma unroll
  for (int i = 0; i < ns; ++i) bad = bad || !fin(e[i]);
#pragma unroll
  for (int i = 0; i < ms; ++i) {
    du[i] = u[i] - rc.ur[i];
    bad = bad || !fin(du[i]);
  }
  bad = row_any(bad);
  const double qc = half_quad_row<ns>(rc.sQ, rc.n, l, e, rc.vec);
  const double rr = half_quad_row<ms>(rc.sR, rc.m, l, du, rc.vec);
  acc += (qc + rr) + rc.w;
  return !bad;
}
template <int SYS>
__device__ __forceinline__ double terminal_cost(const RowCost<SYS>& rc, const Lane& l,
                                                const double* x, bool& ok) {
  constexpr int ns = state_dim(SYS);
  double e[ns];
  wrap_diff<ns>(x, rc.xg, rc.wm, e);
  bool bad = false;
#pragma unroll
  for (int i = 0; i < ns; ++i) bad = bad || !fin(e[i]);
  ok = !row_any(bad) && ok;
  return half_quad_row<ns>(rc.sQf, rc.n, l, e, rc.vec);
}

// cost_timeopt_true of one row's X [N+1][n], U [N][m] at horizon T (T <= N)
template <int SYS>
__device__ double row_cost_true(const RowCost<SYS>& rc, const Lane& l, const double* X,
                                const double* U, int T) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  if (T <= 0) return INFINITY;
  double acc = 0.0;
  bool ok = true;
  double x[ns], u[ms];
  for (int k = 0; k < T; ++k) {
    load_slice<ns>(X + (long long)k * rc.n, l, x);
    load_slice<ms>(U + (long long)k * rc.m, l, u);
    ok = stage_inc<SYS>(rc, l, x, u, acc) && ok;
  }
  load_slice<ns>(X + (long long)T * rc.n, l, x);
  const double t = terminal_cost<SYS>(rc, l, x, ok);
  return ok ? acc + t : INFINITY;
}

// ---------------------------------------------------------------- single step
template <int SYS>
__global__ __launch_bounds__(TPB) void dynamics_kernel(DynC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const long long r = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (r >= a.count) return;
  const Lane l = lane_of(a.P);
  double x[ns], u[ms], xn[ns];
  load_slice<ns>(a.X + r * a.x_stride, l, x);
  load_slice<ms>(a.U + r * a.u_stride, l, u);
  row_step<SYS>(l, x, u, a.P.dt, xn);
  store_slice<ns>(a.Xn + r * a.xn_stride, l, xn);
}

// ---------------------------------------------------------------- rollout
template <int SYS>
__global__ __launch_bounds__(TPB) void rollout_kernel(RolloutC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const long long b = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (b >= a.batch) return;
  const Lane l = lane_of(a.P);
  const int n = a.P.count * ns, m = a.P.count * ms, N = a.N;
  const double* U = a.U + b * (long long)N * m;
  double* X = a.X + b * (long long)(N + 1) * n;
  double x[ns], u[ms], xn[ns];
  load_slice<ns>(a.x0 + b * a.x0_bs, l, x);
  store_slice<ns>(X, l, x);
  int k = 0;
  for (; k < N; ++k) {
    load_slice<ms>(U + (long long)k * m, l, u);
    row_step<SYS>(l, x, u, a.P.dt, xn);
    bool bad = false;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < ns; ++i) {
      bad = bad || !fin(xn[i]);
      ss = fma(xn[i], xn[i], ss);
    }
    const double tot = lane_sum<16>(ss);
    // reference: not finite or np.linalg.norm(xn) > max_state_norm -> X[k+1:] = NaN,
    // on the stacked state (the first lane's copy of the sum decides for the row)
    if (row_any(bad) || row_first(sqrt(tot) > a.max_state_norm)) break;
#pragma unroll
    for (int i = 0; i < ns; ++i) x[i] = xn[i];
    store_slice<ns>(X + (long long)(k + 1) * n, l, x);
  }
#pragma unroll
  for (int i = 0; i < ns; ++i) xn[i] = NAN;
  for (int r = k + 1; r <= N; ++r) store_slice<ns>(X + (long long)r * n, l, xn);
}

// ---------------------------------------------------------------- cost
template <int SYS>
__global__ __launch_bounds__(TPB) void cost_kernel(CostCallC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  __shared__ double sc[kCostLds];
  __shared__ double sv[kRows * kVec];
  const int n = a.P.count * ns, m = a.P.count * ms, N = a.N;
  stage_cost(a.c, n, m, sc);
  const long long b = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (b >= a.batch) return;
  const Lane l = lane_of(a.P);
  const int T = a.T[b];
  double J = NAN;
  if (T <= N) {
    const RowCost<SYS> rc = row_cost_of<SYS>(a.c, a.P, l, b, sc, sv + (threadIdx.x >> 4) * kVec);
    J = row_cost_true<SYS>(rc, l, a.X + b * (long long)(N + 1) * n, a.U + b * (long long)N * m, T);
  }
  if (l.a == 0) a.J[b] = J;
}

// ---------------------------------------------------------------- line search
// pass 1: row b * n_alpha + slot rolls out step size `slot` of problem b; the rows
// after them, one per problem, compute J_old.
template <int SYS>
__global__ __launch_bounds__(TPB) void linesearch_kernel(FwdC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  __shared__ double sc[kCostLds];
  __shared__ double sv[kRows * kVec];
  const int n = a.P.count * ns, m = a.P.count * ms, N = a.N;
  stage_cost(a.c, n, m, sc);
  const long long rg = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  const long long nr = a.batch * a.n_alpha;
  if (rg >= nr + a.batch) return;
  const Lane l = lane_of(a.P);
  const bool roll = rg < nr;
  const long long b = roll ? rg / a.n_alpha : rg - nr;
  const int slot = roll ? (int)(rg - b * a.n_alpha) : a.n_alpha;
  const double* X = a.X + b * (long long)(N + 1) * n;
  const double* U = a.U + b * (long long)N * m;
  const int T = a.T_star[b];
  double* vec = sv + (threadIdx.x >> 4) * kVec;
  const RowCost<SYS> rc = row_cost_of<SYS>(a.c, a.P, l, b, sc, vec);
  if (!roll) {
    const double Jo = T > N ? NAN : row_cost_true<SYS>(rc, l, X, U, T);
    if (l.a == 0) a.J_old[b] = Jo;
    return;
  }
  const bool active = (a.active == nullptr || a.active[b] != 0) && T >= 0 && T <= N;
  double* J = a.Jc + b * a.n_alpha + slot;
  if (!active) {
    if (l.a == 0) *J = NAN;
    return;
  }
  const double alpha = a.alphas[slot];
  const double* K = a.K + b * (long long)N * m * n;
  const double* kf = a.kff + b * (long long)N * m;
  const long long row = (long long)(N + 1) * n + (long long)N * m;
  double* Xc = a.ws + (b * a.n_alpha + slot) * row;
  double* Uc = Xc + (long long)(N + 1) * n;
  double x[ns], u[ms], xn[ns];
  load_slice<ns>(X, l, x);
  store_slice<ns>(Xc, l, x);
  double acc = 0.0;
  bool ok = true;  // finite e / du along the horizon
  for (int k = 0; k < N; ++k) {
    load_slice<ms>(U + (long long)k * m, l, u);
    if (k < T) {
      // U'[k] = U[k] + (K_k dx + alpha k_k)   (solver.py:262-263), dx wrapped
      double xr[ns], dx[ns];
      load_slice<ns>(X + (long long)k * n, l, xr);
      wrap_diff<ns>(x, xr, rc.wm, dx);
      wave_sync();
      store_slice<ns>(vec, l, dx);
      wave_sync();
      if (l.live) {
        const double* Kk = K + (long long)k * m * n;
#pragma unroll
        for (int i = 0; i < ms; ++i) {
          const double* Kr = Kk + (l.a * ms + i) * n;
          double r = 0.0;
          for (int c = 0; c < n; ++c) r = fma(Kr[c], vec[c], r);
          u[i] = u[i] + (r + alpha * kf[(long long)k * m + l.a * ms + i]);
        }
      }
      ok = stage_inc<SYS>(rc, l, x, u, acc) && ok;
    }
    store_slice<ms>(Uc + (long long)k * m, l, u);
    row_step<SYS>(l, x, u, a.P.dt, xn);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < ns; ++i) bad = bad || !fin(xn[i]);
    if (row_any(bad)) {  // rejected step size (solver.py:265-267, 272-274)
      if (l.a == 0) *J = NAN;
      return;
    }
#pragma unroll
    for (int i = 0; i < ns; ++i) x[i] = xn[i];
    store_slice<ns>(Xc + (long long)(k + 1) * n, l, x);
    if (k + 1 == T) acc += terminal_cost<SYS>(rc, l, x, ok);
  }
  if (T == 0) ok = false;  // cost_timeopt_true: T* <= 0 -> inf
  if (l.a == 0) *J = ok ? acc : INFINITY;
}

// pass 2: one workgroup per problem: the first alpha with J' < J_old, then the copy
__global__ __launch_bounds__(TPB) void linesearch_pick_kernel(FwdC a, int n, int m) {
  const long long b = blockIdx.x;
  __shared__ int s_win;
  const int N = a.N;
  if (threadIdx.x == 0) {
    const double Jo = a.J_old[b];
    int win = -1;
    for (int s = 0; s < a.n_alpha; ++s) {
      if (a.Jc[b * a.n_alpha + s] < Jo) {  // NaN (rejected / inactive) never wins
        win = s;
        break;
      }
    }
    const bool active = (a.active == nullptr || a.active[b] != 0);
    a.accepted[b] = active ? win : -2;
    a.J[b] = win >= 0 ? a.Jc[b * a.n_alpha + win] : Jo;
    s_win = win;
  }
  __syncthreads();
  const int win = s_win;
  const long long nx = (long long)(N + 1) * n, nu = (long long)N * m;
  const double* srcX = win >= 0 ? a.ws + (b * a.n_alpha + win) * (nx + nu) : a.X + b * nx;
  const double* srcU = win >= 0 ? srcX + nx : a.U + b * nu;
  double* dX = a.X_new + b * nx;
  double* dU = a.U_new + b * nu;
  for (long long e = threadIdx.x; e < nx; e += TPB) dX[e] = srcX[e];
  for (long long e = threadIdx.x; e < nu; e += TPB) dU[e] = srcU[e];
}

// ---------------------------------------------------------------- linearisation
// row = one (problem, step) pair; lane a = member a
template <int SYS, bool CEN>
__global__ __launch_bounds__(TPB) void linearize_kernel(LinC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const long long g = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (g >= a.batch * a.nuse) return;
  const Lane l = lane_of(a.P);
  const int n = a.P.count * ns, m = a.P.count * ms;
  const long long b = g / a.nuse;
  const int k = (int)(g - b * a.nuse);
  const long long r = b * a.nalloc + k, xr = r + b;
  double x[ns], u[ms];
  load_slice<ns>(a.X + xr * n, l, x);
  load_slice<ms>(a.U + r * m, l, u);
  MemberBase<SYS, CEN> mb;
  mb.fin = true;
  if (l.live) member_base<SYS, CEN>(x, u, a.P.dt, a.epsx, a.relx, mb);
  const bool fleet_fin = !row_any(!mb.fin);
  if (!l.live) return;
#pragma unroll
  for (int i = 0; i < ns; ++i) {
    const long long o = r * n + l.a * ns + i;
    if (a.a_res) a.a_res[o] = mb.f0[i] - a.X[(xr + 1) * n + l.a * ns + i];
    if (a.Fx) a.Fx[o] = mb.f0[i];
  }
  member_rows<SYS, CEN>(l.a, a.P.count, x, u, mb, fleet_fin, a.P.dt, a.epsx, a.epsu, a.relx,
                        a.relu, a.A + r * n * n, a.B + r * n * m);
}

inline unsigned row_grid(long long rows) { return (unsigned)((rows + kRows - 1) / kRows); }

template <int SYS>
hipError_t launch(int which, const void* args, hipStream_t st) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const dim3 blk(TPB);
  switch (which) {
    case 0: {
      const DynC& a = *(const DynC*)args;
      hipLaunchKernelGGL((dynamics_kernel<SYS>), dim3(row_grid(a.count)), blk, 0, st, a);
      break;
    }
    case 1: {
      const RolloutC& a = *(const RolloutC*)args;
      hipLaunchKernelGGL((rollout_kernel<SYS>), dim3(row_grid(a.batch)), blk, 0, st, a);
      break;
    }
    case 2: {
      const LinC& a = *(const LinC*)args;
      const dim3 grid(row_grid(a.batch * (long long)a.nuse));
      if (a.central) hipLaunchKernelGGL((linearize_kernel<SYS, true>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((linearize_kernel<SYS, false>), grid, blk, 0, st, a);
      break;
    }
    case 3: {
      const CostCallC& a = *(const CostCallC*)args;
      hipLaunchKernelGGL((cost_kernel<SYS>), dim3(row_grid(a.batch)), blk, 0, st, a);
      break;
    }
    default: {
      const FwdC& a = *(const FwdC*)args;
      hipLaunchKernelGGL((linesearch_kernel<SYS>), dim3(row_grid(a.batch * (a.n_alpha + 1))),
                         blk, 0, st, a);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(linesearch_pick_kernel, dim3((unsigned)a.batch), blk, 0, st, a,
                         a.P.count * ns, a.P.count * ms);
    }
  }
  return hipGetLastError();
}

hipError_t dispatch(int sys, int which, const void* args, hipStream_t st) {
  switch (sys) {
    case kDI: return launch<kDI>(which, args, st);
    case kCartpole: return launch<kCartpole>(which, args, st);
    case kQuadrotor: return launch<kQuadrotor>(which, args, st);
    case kPointmass: return launch<kPointmass>(which, args, st);
    default: return launch<kSegway>(which, args, st);
  }
}

}  // namespace fleet
}  // namespace hop

// ---------------------------------------------------------------- C entries
namespace {

using hop::set_error;
using hop::fleet::Par;

struct Dims {
  int n, m;
};

int params_of(const hop_fleet_params* q, Par* P, Dims* d) {
  if (!q) return set_error(HOP_E_ARG, "null fleet parameters");
  if (q->system < 0 || q->system >= hop::dyn::kNumSystems)
    return set_error(HOP_E_ARG, "fleet: unknown system (0..4)");
  if (q->count < 1) return set_error(HOP_E_SIZE, "fleet: count must be >= 1");
  if (!hop::fleet::shape_ok(q->system, q->count))
    return set_error(HOP_E_SIZE, "fleet: n must be <= 31 and m <= 16");
  if (!(q->dt > 0.0)) return set_error(HOP_E_ARG, "fleet: dt must be positive");
  *P = Par{q->system, q->count, q->dt};
  d->n = q->count * hop::dyn::state_dim(q->system);
  d->m = q->count * hop::dyn::control_dim(q->system);
  return HOP_OK;
}

int cost_of(const double* xg, int64_t xg_bs, const double* u_ref, int64_t ur_bs, const double* Q,
            const double* R, const double* Qf, const double* w, int64_t w_bs, uint32_t wrap_mask,
            int n, hop::fleet::CostC* c) {
  if (!xg || !u_ref || !Q || !R || !Qf || !w) return set_error(HOP_E_ARG, "null cost parameter");
  if (xg_bs < 0 || ur_bs < 0 || w_bs < 0) return set_error(HOP_E_ARG, "negative batch stride");
  if ((uint64_t)wrap_mask >> n) return set_error(HOP_E_ARG, "wrap bits at or above n");
  *c = hop::fleet::CostC{xg, xg_bs, u_ref, ur_bs, Q, R, Qf, w, w_bs, wrap_mask};
  return HOP_OK;
}

// one launch holds at most 2^32 work-items: rows of 16 lanes, whole workgroups
constexpr int64_t kMaxItems = 0xffffffffLL;
bool rows_fit(int64_t rows) {
  return rows <= kMaxItems / hop::kRowLanes - hop::fleet::kRows;
}

int launched(const Par& P, int which, const void* a, void* stream) {
  return hop::set_hip_status(hop::fleet::dispatch(P.sys, which, a, (hipStream_t)stream));
}

}  // namespace

extern "C" {

int hop_fleet_dynamics_f64(const hop_fleet_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream) {
  hop::fleet::DynC a{};
  Dims d;
  if (int rc = params_of(params, &a.P, &d)) return rc;
  if (count < 0) return set_error(HOP_E_ARG, "count < 0");
  if (count == 0) return HOP_OK;
  if (!X || !U || !Xn) return set_error(HOP_E_ARG, "null input/output pointer");
  if (x_stride < d.n || u_stride < d.m || xn_stride < d.n)
    return set_error(HOP_E_ARG, "row stride too small");
  if (!rows_fit(count)) return set_error(HOP_E_SIZE, "count too large for one launch");
  a.X = X; a.U = U; a.Xn = Xn;
  a.count = count; a.x_stride = x_stride; a.u_stride = u_stride; a.xn_stride = xn_stride;
  return launched(a.P, 0, &a, stream);
}

int hop_fleet_rollout_f64(const hop_fleet_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream) {
  Par P;
  Dims d;
  if (int rc = params_of(params, &P, &d)) return rc;
  if (batch < 0 || N < 0 || x0_batch_stride < 0)
    return set_error(HOP_E_ARG, "negative size/stride");
  if (batch == 0) return HOP_OK;
  if (!x0 || !X || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  hop::fleet::RolloutC a{P, x0, x0_batch_stride, U, batch, N, max_state_norm, X};
  return launched(P, 1, &a, stream);
}

int hop_fleet_linearize_f64(const hop_fleet_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream) {
  hop::fleet::LinC a{};
  Dims d;
  if (int rc = params_of(params, &a.P, &d)) return rc;
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n_alloc < 0) return set_error(HOP_E_ARG, "n_alloc < 0");
  if (n_use > n_alloc) return set_error(HOP_E_ARG, "n_use > n_alloc");
  if (central != 0 && central != 1) return set_error(HOP_E_ARG, "central must be 0 or 1");
  if (batch == 0 || n_use <= 0) return HOP_OK;
  if (!X || !U || !A || !Bm) return set_error(HOP_E_ARG, "null input/output pointer");
  if (batch > kMaxItems || !rows_fit(batch * (int64_t)n_use))
    return set_error(HOP_E_SIZE, "batch * n_use too large for one launch");
  a.central = central;
  a.epsx = epsx; a.epsu = epsu; a.relx = relx; a.relu = relu;
  a.X = X; a.U = U; a.batch = batch; a.nalloc = n_alloc; a.nuse = n_use;
  a.A = A; a.B = Bm; a.a_res = a_res; a.Fx = Fx;
  return launched(a.P, 2, &a, stream);
}

int hop_fleet_cost_true_f64(const hop_fleet_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, uint32_t wrap_mask, int64_t batch,
                            int32_t N, double* J, void* stream) {
  hop::fleet::CostCallC a{};
  Dims d;
  if (int rc = params_of(params, &a.P, &d)) return rc;
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if ((uint64_t)wrap_mask >> d.n) return set_error(HOP_E_ARG, "wrap bits at or above n");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_of(xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                       w_batch_stride, wrap_mask, d.n, &a.c))
    return rc;
  if (!X || !T_star || !J || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  a.X = X; a.U = U; a.T = T_star; a.batch = batch; a.N = N; a.J = J;
  return launched(a.P, 3, &a, stream);
}

size_t hop_fleet_forward_workspace_bytes(const hop_fleet_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha) {
  if (!params || !hop::fleet::shape_ok(params->system, params->count) || batch < 0 || N < 0 ||
      n_alpha < 0)
    return 0;
  const int64_t n = params->count * hop::dyn::state_dim(params->system);
  const int64_t m = params->count * hop::dyn::control_dim(params->system);
  const int64_t row = (int64_t)(N + 1) * n + (int64_t)N * m;
  return (size_t)(batch * n_alpha * (1 + row) * (int64_t)sizeof(double));
}

int hop_fleet_forward_linesearch_f64(const hop_fleet_params* params, const double* X,
                                     const double* U, const double* xg, int64_t xg_batch_stride,
                                     const double* u_ref, int64_t u_ref_batch_stride,
                                     const double* Q, const double* R, const double* Qf,
                                     const double* w, int64_t w_batch_stride, uint32_t wrap_mask,
                                     const int32_t* T_star, const int32_t* active,
                                     const double* K, const double* k, const double* alphas,
                                     int32_t n_alpha, int64_t batch, int32_t N, void* workspace,
                                     size_t workspace_bytes, double* X_new, double* U_new,
                                     double* J, double* J_old, int32_t* accepted, void* stream) {
  hop::fleet::FwdC a{};
  Dims d;
  if (int rc = params_of(params, &a.P, &d)) return rc;
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if (n_alpha < 1 || n_alpha > 8 || !alphas)
    return set_error(HOP_E_ARG, "1 <= n_alpha <= 8 host alphas");
  if ((uint64_t)wrap_mask >> d.n) return set_error(HOP_E_ARG, "wrap bits at or above n");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_of(xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                       w_batch_stride, wrap_mask, d.n, &a.c))
    return rc;
  if (!X || !T_star || !K || !k || !X_new || !U_new || !J || !J_old || !accepted ||
      (N > 0 && !U))
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > kMaxItems / hop::fleet::TPB || !rows_fit(batch * (n_alpha + 1)))
    return set_error(HOP_E_SIZE, "batch too large for one launch");
  const size_t need = hop_fleet_forward_workspace_bytes(params, batch, N, n_alpha);
  if (!workspace || workspace_bytes < need) return set_error(HOP_E_ARG, "workspace too small");
  a.X = X; a.U = U; a.T_star = T_star; a.active = active; a.K = K; a.kff = k;
  for (int i = 0; i < n_alpha; ++i) a.alphas[i] = alphas[i];
  a.n_alpha = n_alpha; a.batch = batch; a.N = N;
  a.Jc = (double*)workspace;
  a.ws = a.Jc + batch * n_alpha;
  a.J_old = J_old; a.X_new = X_new; a.U_new = U_new; a.J = J; a.accepted = accepted;
  return launched(a.P, 4, &a, stream);
}

}  // extern "C"
