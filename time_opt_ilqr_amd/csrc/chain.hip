// The mass-spring chain as a device system (include/hop_chain.h): a wide solve's
// rollout, true cost, forward line search and FD linearisation without the host.
//   chain_dynamics             make_golden_wide.py:54-74  hop_chain_dynamics_f64
//   rollout                    solver.py:42-62            hop_chain_rollout_f64
//   cost_timeopt_true          solver.py:65-102           hop_chain_cost_true_f64
//   forward_linesearch_fixedT  solver.py:233-286          hop_chain_forward_linesearch_f64
//   linearize_*_diff_traj, compute_affine_residuals
//                              linearization.py:177-270   hop_chain_linearize_f64
// p (masses) and m (inputs) are run-time arguments: one instantiation per kernel.
//
// Row layout (everything sequential in time): one trajectory per 16-lane DPP row, four
// per wave64.  Lane i holds mass i -- (q_i, v_i) and the matching entries of x_ref, dx
// and e -- and lanes >= p hold exact zeros.  Lane i evaluates spring i (p + 1 <= 16
// springs: one sin per lane and step); q_{i-1} and f_{i+1} arrive by one-lane DPP row
// shifts, and the zero shifted in at a row's ends is the fixed wall: lane -1's zero and
// the zero that lane p holds both fall out of the layout.  Q e, 0.5 e.Qe, 0.5 du.R du
// and K_k dx are DPP broadcast sums along the row (hop_device.hpp); the shared cost
// blocks sit in LDS, zero-padded to 16 x 16 per block.  The per-step accumulation
// c += (0.5 e.Qe + 0.5 du.R du) + w and the terminal term keep the reference's order;
// the J_old rows and the candidate rows run the same stage function.
//
// Linearisation: one wave per (problem, step).  The base springs and the moved springs
// of every q column (four per column, two for forward differences) are evaluated once
// into LDS; every entry of [A | B] is then a few flops on them (chain_dynamics.hpp,
// chain_out) and the wave stores 64 consecutive entries of the row-major blocks at a
// time with non-temporal stores.
#include <math.h>

#include "hop_device.hpp"
#include "hop_kernels.hpp"
#include "chain_dynamics.hpp"
#include "../../include/hop_chain.h"

namespace hop {
namespace chain {

constexpr int TPB = 256;                 // 16 rows per workgroup
constexpr int kRows = TPB / kRowLanes;
constexpr int kLd = kLdsRow;             // padded LDS row of a 16 x 16 block
constexpr int kBlk = kRowLanes * kLd;    // one padded block
constexpr int kCostLds = 9 * kBlk;       // Q (qq, qv, vq, vv), Qf (the same four), R

struct CostC {
  const double* xg; long long xg_bs;     // [B or 1][n]
  const double* u_ref; long long ur_bs;  // [B or 1][m]
  const double* Q; const double* R; const double* Qf;  // shared
  const double* w; long long w_bs;       // [B or 1]
};
struct DynC {
  Params P;
  const double* X; const double* U; double* Xn;
  long long count, x_stride, u_stride, xn_stride;
};
struct RolloutC {
  Params P;
  const double* x0; long long x0_bs;
  const double* U; long long batch; int N;
  double max_state_norm;
  double* X;
};
struct CostCallC {
  Params P;
  CostC c;
  const double* X; const double* U; const int* T;
  long long batch; int N;
  double* J;
};
struct FwdC {
  Params P;
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
  Params P;
  int central;
  double epsx, epsu, relx, relu;
  const double* X; const double* U;
  long long batch; int nalloc, nuse;
  double* A; double* B; double* a_res; double* Fx;
};

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }

// lane i <- lane i - 1 of its row (lane 0 <- 0) and lane i <- lane i + 1 (lane 15 <- 0)
__device__ __forceinline__ double row_from_below(double v) {
  const int2 w = __builtin_bit_cast(int2, v);
  const int lo = __builtin_amdgcn_update_dpp(0, w.x, 0x111, 0xf, 0xf, true);  // row_shr:1
  const int hi = __builtin_amdgcn_update_dpp(0, w.y, 0x111, 0xf, 0xf, true);
  return __builtin_bit_cast(double, make_int2(lo, hi));
}
__device__ __forceinline__ double row_from_above(double v) {
  const int2 w = __builtin_bit_cast(int2, v);
  const int lo = __builtin_amdgcn_update_dpp(0, w.x, 0x101, 0xf, 0xf, true);  // row_shl:1
  const int hi = __builtin_amdgcn_update_dpp(0, w.y, 0x101, 0xf, 0xf, true);
  return __builtin_bit_cast(double, make_int2(lo, hi));
}

// true on every lane of a row when pred holds on any of its lanes
__device__ __forceinline__ bool row_any(bool pred) {
  const unsigned long long b = __ballot(pred);
  return ((b >> (threadIdx.x & 48)) & 0xffffull) != 0ull;
}

// what a lane is within its row
struct Lane {
  int i;       // lane of the row = mass / spring / input index
  bool mass;   // i < p
  bool inp;    // i < m
  int jact;    // the input that pushes mass i, or -1
};
__device__ __forceinline__ Lane lane_of(const Params& P) {
  Lane l;
  l.i = threadIdx.x & 15;
  l.mass = l.i < P.p;
  l.inp = l.i < P.m;
  l.jact = -1;
  for (int j = 0; j < P.m; ++j)
    if (act_mass(j, P.p, P.m) == l.i) l.jact = j;
  return l;
}

// One Euler step of a row: lane i holds (q_i, v_i), u = the input on this lane's mass.
// The rollout, the line search and the single-step kernel all step through this.
__device__ __forceinline__ void row_step(const Params& P, const Lane& l, double q, double v,
                                         double u, double& qn, double& vn) {
  const double f = spring(stretch(q, row_from_below(q)), P.k, P.ks);  // spring i
  const double fhi = row_from_above(f);                               // spring i + 1
  qn = l.mass ? q_next(q, v, P.dt) : 0.0;
  vn = l.mass ? v_next(v, fhi, f, P.c, P.dt, l.jact >= 0, u) : 0.0;
}

// ---- cost blocks in LDS ------------------------------------------------------
// block t of sc: rows i, columns j of a 16 x 16 zero-padded matrix at [i * kLd + j]
__device__ __forceinline__ void stage_cost(const CostC& c, int p, int m, double* sc, bool& diag) {
  const int n = 2 * p;
  for (int e = threadIdx.x; e < kCostLds; e += TPB) {
    const int t = e / kBlk, r = e - t * kBlk, i = r / kLd, j = r - i * kLd;
    double v = 0.0;
    if (t < 8) {
      if (i < p && j < p) {
        const double* M = t < 4 ? c.Q : c.Qf;
        v = M[(i + ((t >> 1) & 1) * p) * n + j + (t & 1) * p];
      }
    } else if (i < m && j < m) {
      v = c.R[i * m + j];
    }
    sc[e] = v;
  }
  __syncthreads();
  // diagonal Q, Qf and R (every maker's): the cost reads the diagonals only
  bool dg = true;
  for (int e = threadIdx.x; e < kCostLds; e += TPB) {
    const int t = e / kBlk, r = e - t * kBlk, i = r / kLd, j = r - i * kLd;
    const bool on_diag = i == j && (t == 0 || t == 3 || t == 4 || t == 7 || t == 8);
    if (!on_diag && sc[e] != 0.0) dg = false;
  }
  diag = __syncthreads_and(dg) != 0;
}

// 0.5 e.(M e) for M's four padded blocks at sq, e = (eq, ev) on lane i; every lane of
// the row gets the same number
__device__ __forceinline__ double half_quad_x(const double* sq, int i, double eq, double ev,
                                              bool diag) {
  double part;
  if (diag) {
    part = eq * (sq[i * kLd + i] * eq) + ev * (sq[3 * kBlk + i * kLd + i] * ev);
  } else {
    double rq = 0.0, rv = 0.0, y[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = sq[i * kLd + j];
    LaneDot<16>::fma(rq, eq, y);  // rq += sum_j bcast_j(eq) Qqq[i][j]
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = sq[kBlk + i * kLd + j];
    LaneDot<16>::fma(rq, ev, y);
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = sq[2 * kBlk + i * kLd + j];
    LaneDot<16>::fma(rv, eq, y);
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = sq[3 * kBlk + i * kLd + j];
    LaneDot<16>::fma(rv, ev, y);
    part = eq * rq + ev * rv;
  }
  return 0.5 * lane_sum<16>(part);
}

// 0.5 du.(R du), du_j on lane j
__device__ __forceinline__ double half_quad_u(const double* sr, int i, double du, bool diag) {
  double part;
  if (diag) {
    part = du * (sr[i * kLd + i] * du);
  } else {
    double rr = 0.0, y[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = sr[i * kLd + j];
    LaneDot<16>::fma(rr, du, y);
    part = du * rr;
  }
  return 0.5 * lane_sum<16>(part);
}

// what a row needs of the cost: its lane's entries of xg and u_ref, w, the LDS blocks
struct RowCost {
  const double* sc;
  bool diag;
  double xgq, xgv, ur, w;
};
__device__ __forceinline__ RowCost row_cost_of(const CostC& c, const Params& P, const Lane& l,
                                               long long b, const double* sc, bool diag) {
  RowCost r;
  r.sc = sc;
  r.diag = diag;
  const double* xg = c.xg + b * c.xg_bs;
  r.xgq = l.mass ? xg[l.i] : 0.0;
  r.xgv = l.mass ? xg[P.p + l.i] : 0.0;
  r.ur = l.inp ? c.u_ref[b * c.ur_bs + l.i] : 0.0;
  r.w = c.w[b * c.w_bs];
  return r;
}

// running-cost increment of one step (solver.py:87-95): acc += (q + r) + w; returns
// false if e or du is not finite.  (q, v): the state on this lane, u: input `lane`.
__device__ __forceinline__ bool stage_inc(const RowCost& rc, const Lane& l, double q, double v,
                                          double u, double& acc) {
  const double eq = q - rc.xgq, ev = v - rc.xgv, du = u - rc.ur;
  const bool bad = row_any(!fin(eq) || !fin(ev) || !fin(du));
  const double qc = half_quad_x(rc.sc, l.i, eq, ev, rc.diag);
  const double rr = half_quad_u(rc.sc + 8 * kBlk, l.i, du, rc.diag);
  acc += (qc + rr) + rc.w;
  return !bad;
}
__device__ __forceinline__ double terminal_cost(const RowCost& rc, const Lane& l, double q,
                                                double v, bool& ok) {
  const double eq = q - rc.xgq, ev = v - rc.xgv;
  ok = !row_any(!fin(eq) || !fin(ev)) && ok;
  return half_quad_x(rc.sc + 4 * kBlk, l.i, eq, ev, rc.diag);
}

// cost_timeopt_true of one row's X [N+1][n], U [N][m] at horizon T (T <= N)
__device__ double row_cost_true(const RowCost& rc, const Params& P, const Lane& l,
                                const double* X, const double* U, int T) {
  if (T <= 0) return INFINITY;
  const int p = P.p, n = 2 * p, m = P.m;
  double acc = 0.0;
  bool ok = true;
  for (int k = 0; k < T; ++k) {
    const double q = l.mass ? X[(long long)k * n + l.i] : 0.0;
    const double v = l.mass ? X[(long long)k * n + p + l.i] : 0.0;
    const double u = l.inp ? U[(long long)k * m + l.i] : 0.0;
    ok = stage_inc(rc, l, q, v, u, acc) && ok;
  }
  const double q = l.mass ? X[(long long)T * n + l.i] : 0.0;
  const double v = l.mass ? X[(long long)T * n + p + l.i] : 0.0;
  const double t = terminal_cost(rc, l, q, v, ok);
  return ok ? acc + t : INFINITY;
}

// ---------------------------------------------------------------- single step
__global__ __launch_bounds__(TPB) void dynamics_kernel(DynC a) {
  const long long r = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (r >= a.count) return;
  const Params P = a.P;
  const Lane l = lane_of(P);
  const double* x = a.X + r * a.x_stride;
  const double q = l.mass ? x[l.i] : 0.0, v = l.mass ? x[P.p + l.i] : 0.0;
  const double u = l.jact >= 0 ? a.U[r * a.u_stride + l.jact] : 0.0;
  double qn, vn;
  row_step(P, l, q, v, u, qn, vn);
  if (l.mass) {
    double* o = a.Xn + r * a.xn_stride;
    o[l.i] = qn;
    o[P.p + l.i] = vn;
  }
}

// ---------------------------------------------------------------- rollout
__global__ __launch_bounds__(TPB) void rollout_kernel(RolloutC a) {
  const long long b = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (b >= a.batch) return;
  const Params P = a.P;
  const Lane l = lane_of(P);
  const int p = P.p, n = 2 * p, m = P.m, N = a.N;
  const double* U = a.U + b * (long long)N * m;
  double* X = a.X + b * (long long)(N + 1) * n;
  double q = l.mass ? a.x0[b * a.x0_bs + l.i] : 0.0;
  double v = l.mass ? a.x0[b * a.x0_bs + p + l.i] : 0.0;
  if (l.mass) X[l.i] = q, X[p + l.i] = v;
  int k = 0;
  for (; k < N; ++k) {
    const double u = l.jact >= 0 ? U[(long long)k * m + l.jact] : 0.0;
    double qn, vn;
    row_step(P, l, q, v, u, qn, vn);
    const bool bad = row_any(!fin(qn) || !fin(vn));
    const double ss = lane_sum<16>(fma(qn, qn, vn * vn));
    // reference: not finite or np.linalg.norm(xn) > max_state_norm -> X[k+1:] = NaN
    if (bad || sqrt(ss) > a.max_state_norm) break;
    q = qn, v = vn;
    if (l.mass) X[(long long)(k + 1) * n + l.i] = q, X[(long long)(k + 1) * n + p + l.i] = v;
  }
  if (l.mass)
    for (int r = k + 1; r <= N; ++r) X[(long long)r * n + l.i] = NAN, X[(long long)r * n + p + l.i] = NAN;
}

// ---------------------------------------------------------------- cost
__global__ __launch_bounds__(TPB) void cost_kernel(CostCallC a) {
  __shared__ double sc[kCostLds];
  bool diag;
  stage_cost(a.c, a.P.p, a.P.m, sc, diag);
  const long long b = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  if (b >= a.batch) return;
  const Params P = a.P;
  const Lane l = lane_of(P);
  const int n = 2 * P.p, N = a.N;
  const int T = a.T[b];
  double J = NAN;
  if (T <= N) {
    const RowCost rc = row_cost_of(a.c, P, l, b, sc, diag);
    J = row_cost_true(rc, P, l, a.X + b * (long long)(N + 1) * n, a.U + b * (long long)N * P.m, T);
  }
  if (l.i == 0) a.J[b] = J;
}

// ---------------------------------------------------------------- line search
// pass 1: row b * n_alpha + slot rolls out step size `slot` of problem b; the rows
// after them, one per problem, compute J_old.
__global__ __launch_bounds__(TPB) void linesearch_kernel(FwdC a) {
  __shared__ double sc[kCostLds];
  bool diag;
  stage_cost(a.c, a.P.p, a.P.m, sc, diag);
  const long long rg = (long long)blockIdx.x * kRows + (threadIdx.x >> 4);
  const long long nr = a.batch * a.n_alpha;
  if (rg >= nr + a.batch) return;
  const Params P = a.P;
  const Lane l = lane_of(P);
  const int p = P.p, n = 2 * p, m = P.m, N = a.N;
  const bool roll = rg < nr;
  const long long b = roll ? rg / a.n_alpha : rg - nr;
  const int slot = roll ? (int)(rg - b * a.n_alpha) : a.n_alpha;
  const double* X = a.X + b * (long long)(N + 1) * n;
  const double* U = a.U + b * (long long)N * m;
  const int T = a.T_star[b];
  const RowCost rc = row_cost_of(a.c, P, l, b, sc, diag);
  if (!roll) {
    const double Jo = T > N ? NAN : row_cost_true(rc, P, l, X, U, T);
    if (l.i == 0) a.J_old[b] = Jo;
    return;
  }
  const bool active = (a.active == nullptr || a.active[b] != 0) && T >= 0 && T <= N;
  double* J = a.Jc + b * a.n_alpha + slot;
  if (!active) {
    if (l.i == 0) *J = NAN;
    return;
  }
  const double alpha = a.alphas[slot];
  const double* K = a.K + b * (long long)N * m * n;
  const double* kf = a.kff + b * (long long)N * m;
  const long long row = (long long)(N + 1) * n + (long long)N * m;
  double* Xc = a.ws + (b * a.n_alpha + slot) * row;
  double* Uc = Xc + (long long)(N + 1) * n;
  double q = l.mass ? X[l.i] : 0.0, v = l.mass ? X[p + l.i] : 0.0;
  if (l.mass) Xc[l.i] = q, Xc[p + l.i] = v;
  double acc = 0.0;
  bool ok = true;  // finite e / du along the horizon
  for (int k = 0; k < N; ++k) {
    double ul, ua;  // input `lane` (the cost, the U' row) and the input on this lane's mass
    if (k < T) {
      const double dq = l.mass ? q - X[(long long)k * n + l.i] : 0.0;
      const double dv = l.mass ? v - X[(long long)k * n + p + l.i] : 0.0;
      const double* Kk = K + (long long)k * m * n;
      ul = 0.0, ua = 0.0;
      // U'[k] = U[k] + (K_k dx + alpha k_k)   (solver.py:262-263)
      for (int j = 0; j < m; ++j) {
        const double kq = l.mass ? Kk[j * n + l.i] : 0.0, kv = l.mass ? Kk[j * n + p + l.i] : 0.0;
        const double s = lane_sum<16>(fma(kq, dq, kv * dv));
        const double uj = U[(long long)k * m + j] + (s + alpha * kf[(long long)k * m + j]);
        ul = j == l.i ? uj : ul;
        ua = j == l.jact ? uj : ua;
      }
    } else {
      ul = l.inp ? U[(long long)k * m + l.i] : 0.0;
      ua = l.jact >= 0 ? U[(long long)k * m + l.jact] : 0.0;
    }
    if (k < T) ok = stage_inc(rc, l, q, v, ul, acc) && ok;
    if (l.inp) Uc[(long long)k * m + l.i] = ul;
    double qn, vn;
    row_step(P, l, q, v, ua, qn, vn);
    if (row_any(!fin(qn) || !fin(vn))) {  // rejected step size (solver.py:265-267, 272-274)
      if (l.i == 0) *J = NAN;
      return;
    }
    q = qn, v = vn;
    if (l.mass) Xc[(long long)(k + 1) * n + l.i] = q, Xc[(long long)(k + 1) * n + p + l.i] = v;
    if (k + 1 == T) acc += terminal_cost(rc, l, q, v, ok);
  }
  if (T == 0) ok = false;  // cost_timeopt_true: T* <= 0 -> inf
  if (l.i == 0) *J = ok ? acc : INFINITY;
}

// pass 2: one workgroup per problem: the first alpha with J' < J_old, then the copy
__global__ __launch_bounds__(TPB) void linesearch_pick_kernel(FwdC a) {
  const long long b = blockIdx.x;
  __shared__ int s_win;
  const int N = a.N, n = 2 * a.P.p, m = a.P.m;
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
constexpr int kLinWaves = TPB / 64;

template <bool CEN>
__global__ __launch_bounds__(TPB) void linearize_kernel(LinC a) {
  __shared__ double sx[kLinWaves][kMaxN], su[kLinWaves][kMaxP], sf0[kLinWaves][kMaxP + 1],
      sfm[kLinWaves][4 * kMaxP], sF0[kLinWaves][kMaxN], sh[kLinWaves][kMaxN + kMaxP];
  __shared__ int sj[kLinWaves][kMaxP];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * kLinWaves + wv;
  if (g >= a.batch * a.nuse) return;  // a wave without work (no workgroup barrier below)
  const Params P = a.P;
  const int p = P.p, n = 2 * p, m = P.m;
  const long long b = g / a.nuse;
  const int k = (int)(g - b * a.nuse);
  const long long r = b * a.nalloc + k, xr = r + b;
  double* x = sx[wv];
  double* u = su[wv];
  double* f0 = sf0[wv];
  double* fm = sfm[wv];
  double* F0 = sF0[wv];
  double* hc = sh[wv];
  int* jact = sj[wv];
  if (ln < n) x[ln] = a.X[xr * n + ln];
  if (ln < m) u[ln] = a.U[r * m + ln];
  if (ln < p) {
    int ja = 0;  // 1 + input, 0 = none (chain_out)
    for (int j = 0; j < m; ++j)
      if (act_mass(j, p, m) == ln) ja = j + 1;
    jact[ln] = ja;
  }
  wave_sync();
  // the step of every column, the base springs, the moved springs of the q columns
  if (ln < n + m) hc[ln] = col_step(P, x, u, ln, a.epsx, a.epsu, a.relx, a.relu);
  if (ln <= p) f0[ln] = spring(stretch(ln < p ? x[ln] : 0.0, ln > 0 ? x[ln - 1] : 0.0), P.k, P.ks);
  if (ln < 4 * p) {
    const int j = ln >> 2, s = ln & 3;
    if (CEN || s < 2) fm[ln] = moved_spring(P, x, j, s, fd_step(x[j], a.epsx, a.relx));
  }
  wave_sync();
  double Fi = 0.0;
  if (ln < n) {
    Fi = chain_out(P, x, u, f0, fm, jact, ln, -1, 0, 0.0);
    F0[ln] = Fi;
    if (a.a_res) a.a_res[r * n + ln] = Fi - a.X[(xr + 1) * n + ln];
    if (a.Fx) a.Fx[r * n + ln] = Fi;
  }
  const bool f0_finite = __ballot(ln < n && !finite_d(Fi)) == 0ull;
  wave_sync();
  double* A = a.A + r * n * n;
  for (int e = ln; e < n * n; e += 64) {
    const int i = e / n, jj = e - i * n;
    __builtin_nontemporal_store(fd_entry<CEN>(P, x, u, f0, fm, jact, F0, f0_finite, i, jj, hc[jj]),
                                A + e);
  }
  double* B = a.B + r * n * m;
  for (int e = ln; e < n * m; e += 64) {
    const int i = e / m, jj = n + (e - i * m);
    __builtin_nontemporal_store(fd_entry<CEN>(P, x, u, f0, fm, jact, F0, f0_finite, i, jj, hc[jj]),
                                B + e);
  }
  // A step with a non-finite state leaves NaN in this wave's LDS slices, and LDS is not
  // cleared between kernels: a later kernel that reads words it has not written would
  // meet them (the wide Riccati pass did, on the device that ran such a step before it).
  // Leave zeros behind.
  wave_sync();
  auto scrub = [&](double* q, int cnt) {  // volatile: stores nothing reads are not dropped
    if (ln < cnt) ((volatile double*)q)[ln] = 0.0;
  };
  scrub(x, kMaxN), scrub(F0, kMaxN), scrub(u, kMaxP), scrub(f0, kMaxP + 1);
  scrub(fm, 4 * kMaxP), scrub(hc, kMaxN + kMaxP);
}

inline unsigned row_grid(long long rows) { return (unsigned)((rows + kRows - 1) / kRows); }

}  // namespace chain
}  // namespace hop

// ---------------------------------------------------------------- C entries
namespace {

using hop::set_error;
using hop::chain::Params;

int params_of(const hop_chain_params* q, Params* P) {
  if (!q) return set_error(HOP_E_ARG, "null chain parameters");
  if (q->p < 1 || q->p > HOP_CHAIN_MAX_P) return set_error(HOP_E_SIZE, "chain: p must be in [1, 15]");
  if (q->m < 1 || q->m > q->p) return set_error(HOP_E_SIZE, "chain: m must be in [1, p]");
  if (!(q->dt > 0.0)) return set_error(HOP_E_ARG, "chain: dt must be positive");
  *P = Params{q->p, q->m, q->dt, q->k, q->ks, q->c};
  return HOP_OK;
}

int cost_of(const double* xg, int64_t xg_bs, const double* u_ref, int64_t ur_bs, const double* Q,
            const double* R, const double* Qf, const double* w, int64_t w_bs,
            hop::chain::CostC* c) {
  if (!xg || !u_ref || !Q || !R || !Qf || !w) return set_error(HOP_E_ARG, "null cost parameter");
  if (xg_bs < 0 || ur_bs < 0 || w_bs < 0) return set_error(HOP_E_ARG, "negative batch stride");
  *c = hop::chain::CostC{xg, xg_bs, u_ref, ur_bs, Q, R, Qf, w, w_bs};
  return HOP_OK;
}

// one launch holds at most 2^32 work-items: rows of 16 lanes, whole workgroups
constexpr int64_t kMaxItems = 0xffffffffLL;
bool rows_fit(int64_t rows) {
  return rows <= kMaxItems / hop::kRowLanes - hop::chain::kRows;
}

}  // namespace

extern "C" {

int hop_chain_dynamics_f64(const hop_chain_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream) {
  hop::chain::DynC a{};
  if (int rc = params_of(params, &a.P)) return rc;
  if (count < 0) return set_error(HOP_E_ARG, "count < 0");
  if (count == 0) return HOP_OK;
  if (!X || !U || !Xn) return set_error(HOP_E_ARG, "null input/output pointer");
  const int n = 2 * a.P.p;
  if (x_stride < n || u_stride < a.P.m || xn_stride < n)
    return set_error(HOP_E_ARG, "row stride too small");
  if (!rows_fit(count)) return set_error(HOP_E_SIZE, "count too large for one launch");
  a.X = X; a.U = U; a.Xn = Xn;
  a.count = count; a.x_stride = x_stride; a.u_stride = u_stride; a.xn_stride = xn_stride;
  hipLaunchKernelGGL(hop::chain::dynamics_kernel, dim3(hop::chain::row_grid(count)),
                     dim3(hop::chain::TPB), 0, (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

int hop_chain_rollout_f64(const hop_chain_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream) {
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  if (batch < 0 || N < 0 || x0_batch_stride < 0)
    return set_error(HOP_E_ARG, "negative size/stride");
  if (batch == 0) return HOP_OK;
  if (!x0 || !X || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  hop::chain::RolloutC a{P, x0, x0_batch_stride, U, batch, N, max_state_norm, X};
  hipLaunchKernelGGL(hop::chain::rollout_kernel, dim3(hop::chain::row_grid(batch)),
                     dim3(hop::chain::TPB), 0, (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

int hop_chain_linearize_f64(const hop_chain_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream) {
  hop::chain::LinC a{};
  if (int rc = params_of(params, &a.P)) return rc;
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n_use > n_alloc) return set_error(HOP_E_ARG, "n_use > n_alloc");
  if (central != 0 && central != 1) return set_error(HOP_E_ARG, "central must be 0 or 1");
  if (batch == 0 || n_use <= 0) return HOP_OK;
  if (!X || !U || !A || !Bm) return set_error(HOP_E_ARG, "null input/output pointer");
  if (batch > kMaxItems || batch * (int64_t)n_use > kMaxItems / 64 - hop::chain::kLinWaves)
    return set_error(HOP_E_SIZE, "batch * n_use too large for one launch");
  a.central = central;
  a.epsx = epsx; a.epsu = epsu; a.relx = relx; a.relu = relu;
  a.X = X; a.U = U; a.batch = batch; a.nalloc = n_alloc; a.nuse = n_use;
  a.A = A; a.B = Bm; a.a_res = a_res; a.Fx = Fx;
  const int64_t waves = batch * (int64_t)n_use;
  const dim3 grid((unsigned)((waves + hop::chain::kLinWaves - 1) / hop::chain::kLinWaves));
  if (central)
    hipLaunchKernelGGL(hop::chain::linearize_kernel<true>, grid, dim3(hop::chain::TPB), 0,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(hop::chain::linearize_kernel<false>, grid, dim3(hop::chain::TPB), 0,
                       (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

int hop_chain_cost_true_f64(const hop_chain_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, int64_t batch, int32_t N, double* J,
                            void* stream) {
  hop::chain::CostCallC a{};
  if (int rc = params_of(params, &a.P)) return rc;
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_of(xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                       w_batch_stride, &a.c))
    return rc;
  if (!X || !T_star || !J || (N > 0 && !U)) return set_error(HOP_E_ARG, "null pointer");
  if (!rows_fit(batch)) return set_error(HOP_E_SIZE, "batch too large for one launch");
  a.X = X; a.U = U; a.T = T_star; a.batch = batch; a.N = N; a.J = J;
  hipLaunchKernelGGL(hop::chain::cost_kernel, dim3(hop::chain::row_grid(batch)),
                     dim3(hop::chain::TPB), 0, (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

size_t hop_chain_forward_workspace_bytes(const hop_chain_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha) {
  if (!params || params->p < 1 || params->p > HOP_CHAIN_MAX_P || params->m < 1 ||
      params->m > params->p || batch < 0 || N < 0 || n_alpha < 0)
    return 0;
  const int64_t n = 2 * params->p, m = params->m;
  const int64_t row = (int64_t)(N + 1) * n + (int64_t)N * m;
  return (size_t)(batch * n_alpha * (1 + row) * (int64_t)sizeof(double));
}

int hop_chain_forward_linesearch_f64(const hop_chain_params* params, const double* X,
                                     const double* U, const double* xg, int64_t xg_batch_stride,
                                     const double* u_ref, int64_t u_ref_batch_stride,
                                     const double* Q, const double* R, const double* Qf,
                                     const double* w, int64_t w_batch_stride,
                                     const int32_t* T_star, const int32_t* active,
                                     const double* K, const double* k, const double* alphas,
                                     int32_t n_alpha, int64_t batch, int32_t N, void* workspace,
                                     size_t workspace_bytes, double* X_new, double* U_new,
                                     double* J, double* J_old, int32_t* accepted, void* stream) {
  hop::chain::FwdC a{};
  if (int rc = params_of(params, &a.P)) return rc;
  if (batch < 0 || N < 0) return set_error(HOP_E_ARG, "negative size");
  if (n_alpha < 1 || n_alpha > 8 || !alphas)
    return set_error(HOP_E_ARG, "1 <= n_alpha <= 8 host alphas");
  if (batch == 0) return HOP_OK;
  if (int rc = cost_of(xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                       w_batch_stride, &a.c))
    return rc;
  if (!X || !T_star || !K || !k || !X_new || !U_new || !J || !J_old || !accepted ||
      (N > 0 && !U))
    return set_error(HOP_E_ARG, "null pointer");
  if (batch > kMaxItems / hop::chain::TPB || !rows_fit(batch * (n_alpha + 1)))
    return set_error(HOP_E_SIZE, "batch too large for one launch");
  const size_t need = hop_chain_forward_workspace_bytes(params, batch, N, n_alpha);
  if (!workspace || workspace_bytes < need) return set_error(HOP_E_ARG, "workspace too small");
  a.X = X; a.U = U; a.T_star = T_star; a.active = active; a.K = K; a.kff = k;
  for (int i = 0; i < n_alpha; ++i) a.alphas[i] = alphas[i];
  a.n_alpha = n_alpha; a.batch = batch; a.N = N;
  a.Jc = (double*)workspace;
  a.ws = a.Jc + batch * n_alpha;
  a.J_old = J_old; a.X_new = X_new; a.U_new = U_new; a.J = J; a.accepted = accepted;
  hipLaunchKernelGGL(hop::chain::linesearch_kernel,
                     dim3(hop::chain::row_grid(batch * (n_alpha + 1))), dim3(hop::chain::TPB), 0,
                     (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop::set_hip_status(e);
  hipLaunchKernelGGL(hop::chain::linesearch_pick_kernel, dim3((unsigned)batch),
                     dim3(hop::chain::TPB), 0, (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

}  // extern "C"
