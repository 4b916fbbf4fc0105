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
// Row layout (ChainRow, the policy of row_system.hpp's kernels and entries): one
// trajectory per 16-lane DPP row.  Lane i holds mass i -- (q_i, v_i) and the matching
// entries of x_ref, dx and e -- and lanes >= p hold exact zeros.  Lane i evaluates
// spring i (p + 1 <= 16 springs: one sin per lane and step); q_{i-1} and f_{i+1} arrive
// by one-lane DPP row shifts, and the zero shifted in at a row's ends is the fixed wall:
// lane -1's zero and the zero that lane p holds both fall out of the layout.  Q e,
// 0.5 e.Qe, 0.5 du.R du and K_k dx are DPP broadcast sums along the row
// (hop_device.hpp); the shared cost blocks sit in LDS, zero-padded to 16 x 16 per block.
//
// Linearisation: one wave per (problem, step).  The base springs and the moved springs
// of every q column (four per column, two for forward differences) are evaluated once
// into LDS; every entry of [A | B] is then a few flops on them (chain_dynamics.hpp,
// chain_out) and the wave stores 64 consecutive entries of the row-major blocks at a
// time with non-temporal stores.
#include "row_system.hpp"
#include "chain_dynamics.hpp"
#include "../../include/hop_chain.h"

namespace hop {
namespace chain {

using rowsys::CostC;
using rowsys::fin;
using rowsys::row_any;
using rowsys::TPB;

constexpr int kLd = kLdsRow;             // padded LDS row of a 16 x 16 block
constexpr int kBlk = kRowLanes * kLd;    // one padded block
constexpr int kCostLds = 9 * kBlk;       // Q (qq, qv, vq, vv), Qf (the same four), R

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

// r += sum_j bcast_j(e) M[i][j] for the padded block M, e_j on lane j
__device__ __forceinline__ void row_dot(double& r, double e, const double* M, int i) {
  double y[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) y[j] = M[i * kLd + j];
  LaneDot<16>::fma(r, e, y);
}

// 0.5 e.(M e) for M's four padded blocks at sq, e = (eq, ev) on lane i; every lane of
// the row gets the same number
__device__ __forceinline__ double half_quad_x(const double* sq, int i, double eq, double ev,
                                              bool diag) {
  double part;
  if (diag) {
    part = eq * (sq[i * kLd + i] * eq) + ev * (sq[3 * kBlk + i * kLd + i] * ev);
  } else {
    double rq = 0.0, rv = 0.0;
    row_dot(rq, eq, sq, i), row_dot(rq, ev, sq + kBlk, i);
    row_dot(rv, eq, sq + 2 * kBlk, i), row_dot(rv, ev, sq + 3 * kBlk, i);
    part = eq * rq + ev * rv;
  }
  return 0.5 * lane_sum<16>(part);
}

// 0.5 du.(R du), du_j on lane j
__device__ __forceinline__ double half_quad_u(const double* sr, int i, double du, bool diag) {
  double rr = 0.0;
  if (diag) rr = sr[i * kLd + i] * du;
  else row_dot(rr, du, sr, i);
  return 0.5 * lane_sum<16>(du * rr);
}

struct ChainRow {
  using Par = Params;
  HOP_HD static int n(const Par& P) { return 2 * P.p; }
  HOP_HD static int m(const Par& P) { return P.m; }

  // what a lane is within its row
  struct Lane {
    int i;       // lane of the row = mass / spring / input index
    bool mass;   // i < p
    bool inp;    // i < m
    int jact;    // the input that pushes mass i, or -1
  };
  HOP_ROWFN Lane lane_of(const Par& P) {
    const int i = rowsys::row_lane();
    Lane l{i, i < P.p, i < P.m, -1};
    for (int j = 0; j < P.m; ++j)
      if (act_mass(j, P.p, P.m) == l.i) l.jact = j;
    return l;
  }

  struct State { double q, v; };   // mass i
  struct Input { double l, a; };   // input `lane` (the cost, a U row), input on this lane's mass
  // (the index sums in 64 bits: in 32 the cost kernel takes 110 VGPRs, not 80)
  HOP_ROWFN State load_x(const double* x, const Par& P, const Lane& l) {
    return {l.mass ? x[l.i] : 0.0, l.mass ? x[(long long)P.p + l.i] : 0.0};
  }
  HOP_ROWFN void store_x(double* x, const Par& P, const Lane& l, const State& s) {
    if (l.mass) x[l.i] = s.q, x[(long long)P.p + l.i] = s.v;
  }
  HOP_ROWFN State nan_x() { return {NAN, NAN}; }
  HOP_ROWFN bool nonfinite(const State& s) { return !fin(s.q) || !fin(s.v); }
  HOP_ROWFN double norm2(const State& s) { return fma(s.q, s.q, s.v * s.v); }
  HOP_ROWFN Input load_u(const double* u, const Par&, const Lane& l) {
    return {l.inp ? u[l.i] : 0.0, l.jact >= 0 ? u[l.jact] : 0.0};
  }
  HOP_ROWFN void store_u(double* u, const Par&, const Lane& l, const Input& s) {
    if (l.inp) u[l.i] = s.l;
  }

  // One Euler step of a row.  The rollout, the line search and the single-step kernel
  // all step through this.
  HOP_ROWFN State step(const Par& P, const Lane& l, const State& s, const Input& u) {
    const double f = spring(stretch(s.q, row_from_below(s.q)), P.k, P.ks);  // spring i
    const double fhi = row_from_above(f);                                   // spring i + 1
    return {l.mass ? q_next(s.q, s.v, P.dt) : 0.0,
            l.mass ? v_next(s.v, fhi, f, P.c, P.dt, l.jact >= 0, u.a) : 0.0};
  }

  // ---- cost blocks in LDS ----------------------------------------------------
  // block t of sc: rows i, columns j of a 16 x 16 zero-padded matrix at [i * kLd + j]
  struct Lds { double sc[kCostLds]; };
  HOP_ROWFN bool stage(const CostC& c, const Par& P, Lds& lds) {
    const int p = P.p, m = P.m, n = 2 * p;
    double* sc = lds.sc;
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
    return __syncthreads_and(dg) != 0;
  }

  // what a row needs of the cost: its lane's entries of xg and u_ref, w, the LDS blocks
  struct RowCost {
    const double* sc;
    bool diag;
    double xgq, xgv, ur, w;
  };
  HOP_ROWFN RowCost row_cost_of(const CostC& c, const Par& P, const Lane& l, long long b,
                                Lds& lds, bool diag) {
    const double* xg = c.xg + b * c.xg_bs;
    return {lds.sc, diag, l.mass ? xg[l.i] : 0.0, l.mass ? xg[P.p + l.i] : 0.0,
            l.inp ? c.u_ref[b * c.ur_bs + l.i] : 0.0, c.w[b * c.w_bs]};
  }

  // running-cost increment of one step (solver.py:87-95): acc += (q + r) + w; returns
  // false if e or du is not finite
  HOP_ROWFN bool stage_inc(const RowCost& rc, const Lane& l, const State& s, const Input& u,
                           double& acc) {
    const double eq = s.q - rc.xgq, ev = s.v - rc.xgv, du = u.l - rc.ur;
    const bool bad = row_any(!fin(eq) || !fin(ev) || !fin(du));
    const double qc = half_quad_x(rc.sc, l.i, eq, ev, rc.diag);
    const double rr = half_quad_u(rc.sc + 8 * kBlk, l.i, du, rc.diag);
    acc += (qc + rr) + rc.w;
    return !bad;
  }
  HOP_ROWFN double terminal_cost(const RowCost& rc, const Lane& l, const State& s, bool& ok) {
    const double eq = s.q - rc.xgq, ev = s.v - rc.xgv;
    ok = !row_any(!fin(eq) || !fin(ev)) && ok;
    return half_quad_x(rc.sc + 4 * kBlk, l.i, eq, ev, rc.diag);
  }

  // U'[k] = U[k] + (K_k dx + alpha k_k): one DPP broadcast sum per input
  HOP_ROWFN Input feedback(const RowCost&, const Par& P, const Lane& l, const State& s,
                           const double* xref, const double* U, const double* Kk,
                           const double* kf, double alpha) {
    const int p = P.p, n = 2 * p;
    const double dq = l.mass ? s.q - xref[l.i] : 0.0;
    const double dv = l.mass ? s.v - xref[p + l.i] : 0.0;
    Input u{0.0, 0.0};
    for (int j = 0; j < P.m; ++j) {
      const double kq = l.mass ? Kk[j * n + l.i] : 0.0, kv = l.mass ? Kk[j * n + p + l.i] : 0.0;
      const double sum = lane_sum<16>(fma(kq, dq, kv * dv));
      const double uj = U[j] + (sum + alpha * kf[j]);
      u.l = j == l.i ? uj : u.l;
      u.a = j == l.jact ? uj : u.a;
    }
    return u;
  }
};

// ---------------------------------------------------------------- linearisation
using LinC = rowsys::LinC<Params>;
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

static int params_of(const hop_chain_params* q, Params* P) {
  if (!q) return set_error(HOP_E_ARG, "null chain parameters");
  if (q->p < 1 || q->p > HOP_CHAIN_MAX_P) return set_error(HOP_E_SIZE, "chain: p must be in [1, 15]");
  if (q->m < 1 || q->m > q->p) return set_error(HOP_E_SIZE, "chain: m must be in [1, p]");
  if (!(q->dt > 0.0)) return set_error(HOP_E_ARG, "chain: dt must be positive");
  *P = Params{q->p, q->m, q->dt, q->k, q->ks, q->c};
  return HOP_OK;
}

}  // namespace chain
}  // namespace hop

// ---------------------------------------------------------------- C entries
namespace rowsys = hop::rowsys;
using hop::chain::ChainRow;
using hop::chain::Params;
using hop::chain::params_of;

extern "C" {

int hop_chain_dynamics_f64(const hop_chain_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream) {
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  return rowsys::dynamics_entry<ChainRow>(P, X, x_stride, U, u_stride, count, Xn, xn_stride,
                                          stream);
}

int hop_chain_rollout_f64(const hop_chain_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream) {
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  return rowsys::rollout_entry<ChainRow>(P, x0, x0_batch_stride, U, batch, N, max_state_norm, X,
                                         stream);
}

int hop_chain_linearize_f64(const hop_chain_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream) {
  using namespace hop::chain;
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  if (int rc = rowsys::linearize_checks(X, U, batch, n_alloc, n_use, central, A, Bm,
                                        rowsys::kMaxItems / 64 - kLinWaves))  // whole waves
    return rc < 0 ? rc : HOP_OK;
  const LinC a{P, central, epsx, epsu, relx, relu, X, U, batch, n_alloc, n_use, A, Bm, a_res, Fx};
  const int64_t waves = batch * (int64_t)n_use;
  const dim3 grid((unsigned)((waves + kLinWaves - 1) / kLinWaves));
  if (central)
    hipLaunchKernelGGL(linearize_kernel<true>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(linearize_kernel<false>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  return hop::set_hip_status(hipGetLastError());
}

int hop_chain_cost_true_f64(const hop_chain_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, int64_t batch, int32_t N, double* J,
                            void* stream) {
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, 0u};
  return rowsys::cost_entry<ChainRow>(P, X, U, T_star, cost, batch, N, J, stream);
}

size_t hop_chain_forward_workspace_bytes(const hop_chain_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha) {
  if (!params || params->p < 1 || params->p > HOP_CHAIN_MAX_P || params->m < 1 ||
      params->m > params->p)
    return 0;
  return rowsys::workspace_bytes(2 * params->p, params->m, batch, N, n_alpha);
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
  Params P;
  if (int rc = params_of(params, &P)) return rc;
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, 0u};
  return rowsys::linesearch_entry<ChainRow>(P, X, U, cost, T_star, active, K, k, alphas, n_alpha,
                                            batch, N, workspace, workspace_bytes, X_new, U_new, J,
                                            J_old, accepted, stream);
}

}  // extern "C"
