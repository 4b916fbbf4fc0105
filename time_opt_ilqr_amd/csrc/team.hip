// Teams: mixed fleets of the built-in systems as device systems (include/hop_team.h).  Up
// to 15 members, each one of dynamics.hpp's systems and each of its own kind and size,
// stacked member-major and coupled only through the dense cost blocks, so that a joint
// solve of different robots runs its rollout, true cost, forward line search and FD
// linearisation without the host.
//   rollout                    solver.py:42-62            hop_team_rollout_f64
//   cost_timeopt_true          solver.py:65-102           hop_team_cost_true_f64
//   forward_linesearch_fixedT  solver.py:233-286          hop_team_forward_linesearch_f64
//   linearize_*_diff_traj, compute_affine_residuals
//                              linearization.py:177-270   hop_team_linearize_f64
//
// Row layout (TeamRow<NSMAX, MSMAX>, a policy of row_system.hpp's kernels and entries):
// one trajectory -- or one (problem, step) pair of the linearisation -- per 16-lane DPP
// row, lane a = member a, lanes >= count hold exact zeros and evaluate nothing.  Every row
// of a launch has the same composition: the members' kinds and offsets travel by value in
// the parameter block as packed words (team_math.hpp's Shape) that a lane decodes with
// shifts by its lane index, so no array is indexed by the lane.  A lane's state and input
// are NSMAX and MSMAX registers, touched only through unrolled constant indices under
// i < n_s / i < m_s predicates; two instantiations are built, <4, 2> for teams without a
// quadrotor and <12, 4> for teams with one.  A member steps by dyn::eval<SYS> of its own
// kind, picked by a switch on the lane's kind: lanes of different kinds in a row diverge
// there and the wave runs each distinct kind once per step.  What crosses members goes
// through LDS exactly as in fleet.hip (FleetRow): the dense Q, Qf and R of the workgroup
// and one 32-entry exchange vector per row; lane a forms rows xo_a + i of M v by one
// ascending fma chain per row, then its partial sum in ascending i, then lane_sum<16>.
// The order is FleetRow's, so a team of identical members gives the fleet's bits.
//
// Linearisation: lane a evaluates member a's base point and finite-difference columns
// (team_math.hpp, linearize.hip's arithmetic) and writes rows [xo_a, xo_a + n_s) of A_k
// and B_k in full, the off-block entries by the reference's rule.
//
// The proximity cost (include/hop_mixed_proximity.h) is team_proximity.hpp, included below:
// TeamProxRow<NSMAX, MSMAX>, the policy with the cost in stage_inc, and the Taylor kernel.
#include "row_system.hpp"
#include "team_math.hpp"
#include "../../include/hop_team.h"

namespace hop {
namespace team {

using rowsys::CostC;
using rowsys::fin;
using rowsys::kRows;
using rowsys::row_any;
using rowsys::TPB;

constexpr int kVec = 32;                 // a row's exchange vector: n <= 31, m <= 16
constexpr int kCostLds = 2 * kMaxN * kMaxN + kMaxM * kMaxM;  // Q, Qf, R (dense, packed)

struct Par {
  Shape s;
  double dt;
};
// what a lane is within its row: member a, its kind, offsets and sizes (zeros when idle)
struct Lane {
  int a;
  bool live;  // a < count
  int kind, xo, uo, ns, ms;
};

// the lane's `cnt` entries at p + off into K registers, zeros above
template <int K>
__device__ __forceinline__ void load_slice(const double* p, int off, int cnt, double (&v)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = i < cnt ? p[off + i] : 0.0;
}
template <int K>
__device__ __forceinline__ void store_slice(double* p, int off, int cnt, const double (&v)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (i < cnt) p[off + i] = v[i];
}
template <int K>
__device__ __forceinline__ bool any_nonfinite(const double (&v)[K]) {
  bool bad = false;
#pragma unroll
  for (int i = 0; i < K; ++i) bad = bad || !fin(v[i]);
  return bad;
}

// 0.5 v.(M v) for a dense dim x dim block M in LDS, the lane holding v[off .. off + cnt):
// the lanes publish their slices in the row's vector, the lane forms rows off + i of M v.
// Every lane of the row gets the sum, the same bits on each.  FleetRow's order.
template <int K>
__device__ __forceinline__ double half_quad_row(const double* M, int dim, int off, int cnt,
                                                const double (&v)[K], double* vec) {
  wave_sync();  // the vector's readers of the step before are done
  store_slice<K>(vec, off, cnt, v);
  wave_sync();
  double part = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    if (i < cnt) {
      const double* row = M + (off + i) * dim;
      double r = 0.0;
      for (int c = 0; c < dim; ++c) r = fma(row[c], vec[c], r);
      part = fma(v[i], r, part);
    }
  }
  return 0.5 * lane_sum<16>(part);
}

// a - b on the lane's slice, wrapped where the member's mask says so (utils.py:127-137)
template <int K>
__device__ __forceinline__ void wrap_diff(const double* a, const double* b, unsigned wm, int cnt,
                                          double (&e)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double d = a[i] - b[i];
    e[i] = i < cnt ? ((wm >> i) & 1u ? wrap_angle(d) : d) : 0.0;
  }
}

template <int NSMAX, int MSMAX>
struct TeamRow {
  static constexpr bool kQuad = NSMAX >= state_dim(kQuadrotor);
  using Par = team::Par;
  using Lane = team::Lane;
  HOP_HD static int n(const Par& P) { return P.s.n; }
  HOP_HD static int m(const Par& P) { return P.s.m; }
  HOP_ROWFN Lane lane_of(const Par& P) {
    Lane l;
    l.a = rowsys::row_lane();
    l.live = l.a < P.s.count;
    l.kind = l.live ? kind_of(P.s, l.a) : 0;
    l.xo = l.live ? xo_of(P.s, l.a) : 0;
    l.uo = l.live ? uo_of(P.s, l.a) : 0;
    l.ns = l.live ? state_dim(l.kind) : 0;
    l.ms = l.live ? control_dim(l.kind) : 0;
    return l;
  }

  struct State { double v[NSMAX]; };  // member a, zeros at and above n_s
  struct Input { double v[MSMAX]; };
  HOP_ROWFN State load_x(const double* x, const Par&, const Lane& l) {
    State s;
    load_slice<NSMAX>(x, l.xo, l.ns, s.v);
    return s;
  }
  HOP_ROWFN void store_x(double* x, const Par&, const Lane& l, const State& s) {
    store_slice<NSMAX>(x, l.xo, l.ns, s.v);
  }
  HOP_ROWFN State nan_x() {
    State s;
#pragma unroll
    for (int i = 0; i < NSMAX; ++i) s.v[i] = NAN;
    return s;
  }
  HOP_ROWFN bool nonfinite(const State& s) { return any_nonfinite<NSMAX>(s.v); }
  // the entries at and above n_s are zeros: fma(0, 0, ss) leaves ss as it is
  HOP_ROWFN double norm2(const State& s) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < NSMAX; ++i) ss = fma(s.v[i], s.v[i], ss);
    return ss;
  }
  HOP_ROWFN Input load_u(const double* u, const Par&, const Lane& l) {
    Input s;
    load_slice<MSMAX>(u, l.uo, l.ms, s.v);
    return s;
  }
  HOP_ROWFN void store_u(double* u, const Par&, const Lane& l, const Input& s) {
    store_slice<MSMAX>(u, l.uo, l.ms, s.v);
  }

  // One step of a row: member a on lane a by its own kind's arithmetic; idle lanes and
  // the entries above n_s keep zeros.  The rollout, the line search and the single-step
  // kernel all step through this.  Lanes of different kinds part here and meet again
  // after it.
  HOP_ROWFN State step(const Par& P, const Lane& l, const State& s, const Input& u) {
    State sn;
#pragma unroll
    for (int i = 0; i < NSMAX; ++i) sn.v[i] = 0.0;
    if (l.live) {
      switch (l.kind) {
        case kDI: eval<kDI>(s.v, u.v, P.dt, sn.v); break;
        case kCartpole: eval<kCartpole>(s.v, u.v, P.dt, sn.v); break;
        case kQuadrotor:
          if constexpr (kQuad) eval<kQuadrotor>(s.v, u.v, P.dt, sn.v);
          break;
        case kPointmass: eval<kPointmass>(s.v, u.v, P.dt, sn.v); break;
        default: eval<kSegway>(s.v, u.v, P.dt, sn.v); break;
      }
    }
    return sn;
  }

  // ---- cost blocks in LDS: FleetRow's layout -----------------------------------
  // sc: Q [n][n], then Qf [n][n], then R [m][m], packed; sv: the rows' exchange vectors,
  // first, the struct 16-byte aligned (128-bit LDS reads in the dot products)
  struct alignas(16) Lds { double sv[kRows * kVec], sc[kCostLds]; };
  HOP_ROWFN bool stage(const CostC& c, const Par& P, Lds& lds) {
    const int nq = n(P) * n(P), tot = 2 * nq + m(P) * m(P);
    for (int e = threadIdx.x; e < tot; e += TPB)
      lds.sc[e] = e < nq ? c.Q[e] : e < 2 * nq ? c.Qf[e - nq] : c.R[e - 2 * nq];
    __syncthreads();
    return false;  // no fast path
  }

  // what a row needs of the cost: its lane's entries of xg and u_ref, its wrap bits, w,
  // the LDS blocks and the row's exchange vector
  struct RowCost {
    const double* sQ; const double* sQf; const double* sR;
    double* vec;
    int n, m;
    unsigned wm;  // bits [xo, xo + n_s) of the wrap mask
    double xg[NSMAX], ur[MSMAX], w;
  };
  HOP_ROWFN RowCost row_cost_of(const CostC& c, const Par& P, const Lane& l, long long b,
                                Lds& lds, bool) {
    RowCost r;
    r.n = P.s.n, r.m = P.s.m;
    r.sQ = lds.sc, r.sQf = lds.sc + r.n * r.n, r.sR = lds.sc + 2 * r.n * r.n;
    r.vec = lds.sv + (threadIdx.x >> 4) * kVec;
    r.wm = (c.wrap_mask >> l.xo) & ((1u << l.ns) - 1u);
    load_slice<NSMAX>(c.xg + b * c.xg_bs, l.xo, l.ns, r.xg);
    load_slice<MSMAX>(c.u_ref + b * c.ur_bs, l.uo, l.ms, r.ur);
    r.w = c.w[b * c.w_bs];
    return r;
  }

  // running-cost increment of one step (solver.py:87-95): acc += (q + r) + w; returns
  // false if e or du is not finite in any member
  HOP_ROWFN bool stage_inc(const RowCost& rc, const Lane& l, const State& s, const Input& u,
                           double& acc) {
    double e[NSMAX], du[MSMAX];
    wrap_diff<NSMAX>(s.v, rc.xg, rc.wm, l.ns, e);
#pragma unroll
    for (int i = 0; i < MSMAX; ++i) du[i] = u.v[i] - rc.ur[i];
    const bool bad = row_any(any_nonfinite<NSMAX>(e) || any_nonfinite<MSMAX>(du));
    const double qc = half_quad_row<NSMAX>(rc.sQ, rc.n, l.xo, l.ns, e, rc.vec);
    const double rr = half_quad_row<MSMAX>(rc.sR, rc.m, l.uo, l.ms, du, rc.vec);
    acc += (qc + rr) + rc.w;
    return !bad;
  }
  HOP_ROWFN double terminal_cost(const RowCost& rc, const Lane& l, const State& s, bool& ok) {
    double e[NSMAX];
    wrap_diff<NSMAX>(s.v, rc.xg, rc.wm, l.ns, e);
    ok = !row_any(any_nonfinite<NSMAX>(e)) && ok;
    return half_quad_row<NSMAX>(rc.sQf, rc.n, l.xo, l.ns, e, rc.vec);
  }

  // U'[k] = U[k] + (K_k dx + alpha k_k), dx wrapped: the lanes publish dx in the row's
  // vector and lane a forms member a's rows of K_k dx
  HOP_ROWFN Input feedback(const RowCost& rc, const Par& P, const Lane& l, const State& s,
                           const double* xref, const double* U, const double* Kk,
                           const double* kf, double alpha) {
    Input u = load_u(U, P, l);
    double xr[NSMAX], dx[NSMAX];
    load_slice<NSMAX>(xref, l.xo, l.ns, xr);
    wrap_diff<NSMAX>(s.v, xr, rc.wm, l.ns, dx);
    wave_sync();
    store_slice<NSMAX>(rc.vec, l.xo, l.ns, dx);
    wave_sync();
#pragma unroll
    for (int i = 0; i < MSMAX; ++i) {
      if (i < l.ms) {
        const double* Kr = Kk + (l.uo + i) * rc.n;
        double r = 0.0;
        for (int c = 0; c < rc.n; ++c) r = fma(Kr[c], rc.vec[c], r);
        u.v[i] = u.v[i] + (r + alpha * kf[l.uo + i]);
      }
    }
    return u;
  }
};

// ---------------------------------------------------------------- linearisation
// row = one (problem, step) pair; lane a = member a
using LinC = rowsys::LinC<Par>;

// a member's base point in registers sized for any kind of the instantiation, so that it
// survives the row's vote between the two switches on the kind
template <int NSMAX, bool CEN>
struct AnyBase {
  static constexpr int TS = NSMAX >= state_dim(kQuadrotor) ? trig_slots(kQuadrotor, CEN) : 1;
  double ts[TS], f0[NSMAX];
  bool fin;
};

template <int SYS, bool CEN, int NSMAX>
__device__ __forceinline__ void base_of(const double* x, const double* u, const LinC& a,
                                        AnyBase<NSMAX, CEN>& g) {
  MemberBase<SYS, CEN> mb;
  member_base<SYS, CEN>(x, u, a.P.dt, a.epsx, a.relx, mb);
#pragma unroll
  for (int i = 0; i < MemberBase<SYS, CEN>::TS; ++i) g.ts[i] = mb.ts[i];
#pragma unroll
  for (int i = 0; i < state_dim(SYS); ++i) g.f0[i] = mb.f0[i];
  g.fin = mb.fin;
}

template <int SYS, bool CEN, int NSMAX>
__device__ __forceinline__ void rows_of(const Lane& l, const double* x, const double* u,
                                        const AnyBase<NSMAX, CEN>& g, bool team_fin,
                                        const LinC& a, long long r, long long xr) {
  const int n = a.P.s.n, m = a.P.s.m;
  MemberBase<SYS, CEN> mb;
#pragma unroll
  for (int i = 0; i < MemberBase<SYS, CEN>::TS; ++i) mb.ts[i] = g.ts[i];
#pragma unroll
  for (int i = 0; i < state_dim(SYS); ++i) mb.f0[i] = g.f0[i];
  mb.fin = g.fin;
#pragma unroll
  for (int i = 0; i < state_dim(SYS); ++i) {
    const long long o = r * n + l.xo + i;
    if (a.a_res) a.a_res[o] = mb.f0[i] - a.X[(xr + 1) * n + l.xo + i];
    if (a.Fx) a.Fx[o] = mb.f0[i];
  }
  member_rows<SYS, CEN>(l.xo, l.uo, n, m, x, u, mb, team_fin, a.P.dt, a.epsx, a.epsu, a.relx,
                        a.relu, a.A + r * n * n, a.B + r * n * m);
}

template <int NSMAX, int MSMAX, bool CEN>
__global__ __launch_bounds__(TPB) void linearize_kernel(LinC a) {
  using Row = TeamRow<NSMAX, MSMAX>;
  const long long g = rowsys::row_index();
  if (g >= a.batch * a.nuse) return;
  const Lane l = Row::lane_of(a.P);
  const int n = a.P.s.n, m = a.P.s.m;
  const long long b = g / a.nuse;
  const int k = (int)(g - b * a.nuse);
  const long long r = b * a.nalloc + k, xr = r + b;
  double x[NSMAX], u[MSMAX];
  load_slice<NSMAX>(a.X + xr * n, l.xo, l.ns, x);
  load_slice<MSMAX>(a.U + r * m, l.uo, l.ms, u);
  AnyBase<NSMAX, CEN> mb;
#pragma unroll
  for (int i = 0; i < AnyBase<NSMAX, CEN>::TS; ++i) mb.ts[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NSMAX; ++i) mb.f0[i] = 0.0;
  mb.fin = true;
  if (l.live) {
    switch (l.kind) {
      case kDI: base_of<kDI, CEN>(x, u, a, mb); break;
      case kCartpole: base_of<kCartpole, CEN>(x, u, a, mb); break;
      case kQuadrotor:
        if constexpr (Row::kQuad) base_of<kQuadrotor, CEN>(x, u, a, mb);
        break;
      case kPointmass: base_of<kPointmass, CEN>(x, u, a, mb); break;
      default: base_of<kSegway, CEN>(x, u, a, mb); break;
    }
  }
  const bool team_fin = !row_any(!mb.fin);
  if (!l.live) return;
  switch (l.kind) {
    case kDI: rows_of<kDI, CEN>(l, x, u, mb, team_fin, a, r, xr); break;
    case kCartpole: rows_of<kCartpole, CEN>(l, x, u, mb, team_fin, a, r, xr); break;
    case kQuadrotor:
      if constexpr (Row::kQuad) rows_of<kQuadrotor, CEN>(l, x, u, mb, team_fin, a, r, xr);
      break;
    case kPointmass: rows_of<kPointmass, CEN>(l, x, u, mb, team_fin, a, r, xr); break;
    default: rows_of<kSegway, CEN>(l, x, u, mb, team_fin, a, r, xr); break;
  }
}

template <int NSMAX, int MSMAX>
int launch_linearize(TeamRow<NSMAX, MSMAX>, const LinC& a, hipStream_t st) {
  const dim3 grid(rowsys::row_grid(a.batch * (long long)a.nuse));
  if (a.central)
    hipLaunchKernelGGL((linearize_kernel<NSMAX, MSMAX, true>), grid, dim3(TPB), 0, st, a);
  else
    hipLaunchKernelGGL((linearize_kernel<NSMAX, MSMAX, false>), grid, dim3(TPB), 0, st, a);
  return set_hip_status(hipGetLastError());
}

static int params_of(const hop_team_params* q, Par* P) {
  if (!q) return set_error(HOP_E_ARG, "null team parameters");
  switch (shape_of(q->count, q->system, &P->s)) {
    case 0: break;
    case 1: return set_error(HOP_E_SIZE, "team: count must be in [1, 15]");
    case 2: return set_error(HOP_E_ARG, "team: unknown member system (0..4)");
    default: return set_error(HOP_E_SIZE, "team: n must be <= 31 and m <= 16");
  }
  if (!(q->dt > 0.0)) return set_error(HOP_E_ARG, "team: dt must be positive");
  P->dt = q->dt;
  return HOP_OK;
}

// f(TeamRow<...>{}, P) for the validated parameters: every entry's first step
template <class F>
int with_team(const hop_team_params* q, F&& f) {
  Par P;
  if (int rc = params_of(q, &P)) return rc;
  if (P.s.quad) return f(TeamRow<12, 4>{}, P);
  return f(TeamRow<4, 2>{}, P);
}

}  // namespace team
}  // namespace hop

// the proximity cost: TeamProxRow<NSMAX, MSMAX> and the Taylor kernel
// (hop_mixed_proximity.h)
#include "../../include/hop_mixed_proximity.h"
#include "team_proximity.hpp"

// ---------------------------------------------------------------- C entries
namespace rowsys = hop::rowsys;
using hop::team::Par;
using hop::team::ProxPar;
using hop::team::with_mixed_prox;
using hop::team::with_team;

extern "C" {

int hop_team_dynamics_f64(const hop_team_params* params, const double* X, int64_t x_stride,
                          const double* U, int64_t u_stride, int64_t count, double* Xn,
                          int64_t xn_stride, void* stream) {
  return with_team(params, [&](auto s, const Par& P) {
    return rowsys::dynamics_entry<decltype(s)>(P, X, x_stride, U, u_stride, count, Xn, xn_stride,
                                               stream);
  });
}

int hop_team_rollout_f64(const hop_team_params* params, const double* x0,
                         int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                         double max_state_norm, double* X, void* stream) {
  return with_team(params, [&](auto s, const Par& P) {
    return rowsys::rollout_entry<decltype(s)>(P, x0, x0_batch_stride, U, batch, N,
                                              max_state_norm, X, stream);
  });
}

int hop_team_linearize_f64(const hop_team_params* params, const double* X, const double* U,
                           int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                           double epsx, double epsu, double relx, double relu, double* A,
                           double* Bm, double* a_res, double* Fx, void* stream) {
  return with_team(params, [&](auto s, const Par& P) {
    if (int rc = rowsys::linearize_checks(X, U, batch, n_alloc, n_use, central, A, Bm,
                                          rowsys::kMaxRows))  // one row per (problem, step)
      return rc < 0 ? rc : (int)HOP_OK;
    const hop::team::LinC a{P,     central, epsx,  epsu, relx, relu,  X, U,
                            batch, n_alloc, n_use, A,    Bm,   a_res, Fx};
    return hop::team::launch_linearize(s, a, (hipStream_t)stream);
  });
}

int hop_team_cost_true_f64(const hop_team_params* params, const double* X, const double* U,
                           const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                           const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                           const double* R, const double* Qf, const double* w,
                           int64_t w_batch_stride, uint32_t wrap_mask, int64_t batch,
                           int32_t N, double* J, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_team(params, [&](auto s, const Par& P) {
    return rowsys::cost_entry<decltype(s)>(P, X, U, T_star, cost, batch, N, J, stream);
  });
}

size_t hop_team_forward_workspace_bytes(const hop_team_params* params, int64_t batch,
                                        int32_t N, int32_t n_alpha) {
  hop::team::Shape s;
  if (!params || hop::team::shape_of(params->count, params->system, &s)) return 0;
  return rowsys::workspace_bytes(s.n, s.m, batch, N, n_alpha);
}

int hop_team_forward_linesearch_f64(const hop_team_params* params, const double* X,
                                    const double* U, const double* xg, int64_t xg_batch_stride,
                                    const double* u_ref, int64_t u_ref_batch_stride,
                                    const double* Q, const double* R, const double* Qf,
                                    const double* w, int64_t w_batch_stride, uint32_t wrap_mask,
                                    const int32_t* T_star, const int32_t* active,
                                    const double* K, const double* k, const double* alphas,
                                    int32_t n_alpha, int64_t batch, int32_t N, void* workspace,
                                    size_t workspace_bytes, double* X_new, double* U_new,
                                    double* J, double* J_old, int32_t* accepted, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_team(params, [&](auto s, const Par& P) {
    return rowsys::linesearch_entry<decltype(s)>(P, X, U, cost, T_star, active, K, k, alphas,
                                                 n_alpha, batch, N, workspace, workspace_bytes,
                                                 X_new, U_new, J, J_old, accepted, stream);
  });
}

// ---- include/hop_mixed_proximity.h
int hop_mixed_proximity_taylor_f64(int32_t members, const int32_t* system,
                                   const hop_fleet_proximity* prox, const double* X,
                                   int64_t x_stride, int64_t count, double* c, double* cx,
                                   double* cxx, void* stream) {
  return with_mixed_prox(members, system, false, 0.0, prox, [&](auto, const ProxPar& P) {
    return hop::team::taylor_entry(P, X, x_stride, count, c, cx, cxx, stream);
  });
}

int hop_mixed_prox_cost_true_f64(int32_t members, const int32_t* system, const double* X,
                                 const double* U, const int32_t* T_star, const double* xg,
                                 int64_t xg_batch_stride, const double* u_ref,
                                 int64_t u_ref_batch_stride, const double* Q, const double* R,
                                 const double* Qf, const double* w, int64_t w_batch_stride,
                                 uint32_t wrap_mask, const hop_fleet_proximity* prox,
                                 int64_t batch, int32_t N, double* J, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_mixed_prox(members, system, false, 0.0, prox, [&](auto s, const ProxPar& P) {
    return rowsys::cost_entry<decltype(s)>(P, X, U, T_star, cost, batch, N, J, stream);
  });
}

int hop_mixed_prox_forward_linesearch_f64(
    int32_t members, const int32_t* system, double dt, const double* X, const double* U,
    const double* xg, int64_t xg_batch_stride, const double* u_ref, int64_t u_ref_batch_stride,
    const double* Q, const double* R, const double* Qf, const double* w, int64_t w_batch_stride,
    uint32_t wrap_mask, const hop_fleet_proximity* prox, const int32_t* T_star,
    const int32_t* active, const double* K, const double* k, const double* alphas,
    int32_t n_alpha, int64_t batch, int32_t N, void* workspace, size_t workspace_bytes,
    double* X_new, double* U_new, double* J, double* J_old, int32_t* accepted, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_mixed_prox(members, system, true, dt, prox, [&](auto s, const ProxPar& P) {
    return rowsys::linesearch_entry<decltype(s)>(P, X, U, cost, T_star, active, K, k, alphas,
                                                 n_alpha, batch, N, workspace, workspace_bytes,
                                                 X_new, U_new, J, J_old, accepted, stream);
  });
}

}  // extern "C"
