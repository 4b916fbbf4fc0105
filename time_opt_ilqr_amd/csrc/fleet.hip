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
// Row layout (FleetRow<SYS>, the policy of row_system.hpp's kernels and entries): one
// trajectory -- or one (problem, step) pair of the linearisation -- per 16-lane DPP row.
// Lane a holds member a: its n_s states and m_s inputs, the matching entries of xg,
// u_ref, e, du and dx, and its bits of the wrap mask; lanes >= count hold exact zeros
// and evaluate nothing.  A member steps by dyn::eval<SYS> on its own lane, so a fleet
// step is bit for bit the members' steps.  What crosses members goes through LDS: the
// dense Q, Qf and R of the workgroup, and one 32-entry vector per row into which the
// lanes write their slices of e, du or dx; lane a then forms its own rows of Q e, R du
// or K_k dx from the whole vector (one ascending fma chain per row) and the row sums
// v.(M v) and the squared state norm with hop_device.hpp's lane_sum.
//
// Linearisation: lane a evaluates member a's base point and finite-difference columns
// (fleet_math.hpp, linearize.hip's arithmetic) and writes rows [a n_s, (a + 1) n_s) of
// A_k and B_k in full, the off-block entries by the reference's rule.
//
// The proximity cost (include/hop_fleet_proximity.h) is fleet_proximity.hpp, included below:
// FleetProxRow<SYS>, the policy with the cost in stage_inc, and the Taylor kernel.
#include "row_system.hpp"
#include "fleet_math.hpp"
#include "../../include/hop_fleet.h"

namespace hop {
namespace fleet {

using rowsys::CostC;
using rowsys::fin;
using rowsys::kRows;
using rowsys::row_any;
using rowsys::TPB;

constexpr int kVec = 32;                 // a row's exchange vector: n <= 31, m <= 16
constexpr int kCostLds = 2 * kMaxN * kMaxN + kMaxM * kMaxM;  // Q, Qf, R (dense, packed)

struct Par {
  int sys, count;
  double dt;
};
// what a lane is within its row
struct Lane {
  int a;      // lane of the row = member
  bool live;  // a < count
};

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
template <int K>
__device__ __forceinline__ bool any_nonfinite(const double (&v)[K]) {
  bool bad = false;
#pragma unroll
  for (int i = 0; i < K; ++i) bad = bad || !fin(v[i]);
  return bad;
}

// 0.5 v.(M v) for a dense dim x dim block M in LDS, lane a holding v[a K .. a K + K):
// the lanes publish their slices in the row's vector, lane a forms rows a K .. of M v.
// Every lane of the row gets the sum, the same bits on each (lane_sum runs one
// broadcast-FMA chain on all of them).
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

template <int SYS>
struct FleetRow {
  static constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  using Par = fleet::Par;
  using Lane = fleet::Lane;
  HOP_HD static int n(const Par& P) { return P.count * ns; }
  HOP_HD static int m(const Par& P) { return P.count * ms; }
  HOP_ROWFN Lane lane_of(const Par& P) {
    return {rowsys::row_lane(), rowsys::row_lane() < P.count};
  }

  struct State { double v[ns]; };  // member a
  struct Input { double v[ms]; };
  template <class V>  // State or Input from the lane's slice of a row
  HOP_ROWFN V load(const double* p, const Lane& l) {
    V s;
    load_slice(p, l, s.v);
    return s;
  }
  HOP_ROWFN State load_x(const double* x, const Par&, const Lane& l) { return load<State>(x, l); }
  HOP_ROWFN void store_x(double* x, const Par&, const Lane& l, const State& s) {
    store_slice<ns>(x, l, s.v);
  }
  HOP_ROWFN State nan_x() {
    State s;
#pragma unroll
    for (int i = 0; i < ns; ++i) s.v[i] = NAN;
    return s;
  }
  HOP_ROWFN bool nonfinite(const State& s) { return any_nonfinite<ns>(s.v); }
  HOP_ROWFN double norm2(const State& s) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < ns; ++i) ss = fma(s.v[i], s.v[i], ss);
    return ss;
  }
  HOP_ROWFN Input load_u(const double* u, const Par&, const Lane& l) { return load<Input>(u, l); }
  HOP_ROWFN void store_u(double* u, const Par&, const Lane& l, const Input& s) {
    store_slice<ms>(u, l, s.v);
  }

  // One step of a row: member a on lane a; idle lanes keep zeros.  The rollout, the line
  // search and the single-step kernel all step through this.
  HOP_ROWFN State step(const Par& P, const Lane& l, const State& s, const Input& u) {
    State sn;
#pragma unroll
    for (int i = 0; i < ns; ++i) sn.v[i] = 0.0;
    if (l.live) eval<SYS>(s.v, u.v, P.dt, sn.v);
    return sn;
  }

  // ---- cost blocks in LDS ----------------------------------------------------
  // sc: Q [n][n], then Qf [n][n], then R [m][m], packed; sv: the rows' exchange vectors.
  // 16-byte aligned, or the dot products' 128-bit LDS reads become pairs of 64-bit ones
  // (1.2 to 1.6 x the time); sv first costs fewer registers (profiles/rowsys_regs.txt)
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
    unsigned wm;  // bits [a n_s, (a + 1) n_s) of the wrap mask
    double xg[ns], ur[ms], w;
  };
  HOP_ROWFN RowCost row_cost_of(const CostC& c, const Par& P, const Lane& l, long long b,
                                Lds& lds, bool) {
    RowCost r;
    r.n = P.count * ns, r.m = P.count * ms;
    r.sQ = lds.sc, r.sQf = lds.sc + r.n * r.n, r.sR = lds.sc + 2 * r.n * r.n;
    r.vec = lds.sv + (threadIdx.x >> 4) * kVec;
    r.wm = l.live ? (c.wrap_mask >> (l.a * ns)) & ((1u << ns) - 1u) : 0u;
    load_slice<ns>(c.xg + b * c.xg_bs, l, r.xg);
    load_slice<ms>(c.u_ref + b * c.ur_bs, l, r.ur);
    r.w = c.w[b * c.w_bs];
    return r;
  }

  // running-cost increment of one step (solver.py:87-95): acc += (q + r) + w; returns
  // false if e or du is not finite in any member
  HOP_ROWFN bool stage_inc(const RowCost& rc, const Lane& l, const State& s, const Input& u,
                           double& acc) {
    double e[ns], du[ms];
    wrap_diff<ns>(s.v, rc.xg, rc.wm, e);
#pragma unroll
    for (int i = 0; i < ms; ++i) du[i] = u.v[i] - rc.ur[i];
    const bool bad = row_any(any_nonfinite<ns>(e) || any_nonfinite<ms>(du));
    const double qc = half_quad_row<ns>(rc.sQ, rc.n, l, e, rc.vec);
    const double rr = half_quad_row<ms>(rc.sR, rc.m, l, du, rc.vec);
    acc += (qc + rr) + rc.w;
    return !bad;
  }
  HOP_ROWFN double terminal_cost(const RowCost& rc, const Lane& l, const State& s, bool& ok) {
    double e[ns];
    wrap_diff<ns>(s.v, rc.xg, rc.wm, e);
    ok = !row_any(any_nonfinite<ns>(e)) && ok;
    return half_quad_row<ns>(rc.sQf, rc.n, l, e, rc.vec);
  }

  // U'[k] = U[k] + (K_k dx + alpha k_k), dx wrapped: the lanes publish dx in the row's
  // vector and lane a forms member a's rows of K_k dx
  HOP_ROWFN Input feedback(const RowCost& rc, const Par& P, const Lane& l, const State& s,
                           const double* xref, const double* U, const double* Kk,
                           const double* kf, double alpha) {
    Input u = load_u(U, P, l);
    double xr[ns], dx[ns];
    load_slice<ns>(xref, l, xr);
    wrap_diff<ns>(s.v, xr, rc.wm, dx);
    wave_sync();
    store_slice<ns>(rc.vec, l, dx);
    wave_sync();
    if (l.live) {
#pragma unroll
      for (int i = 0; i < ms; ++i) {
        const double* Kr = Kk + (l.a * ms + i) * rc.n;
        double r = 0.0;
        for (int c = 0; c < rc.n; ++c) r = fma(Kr[c], rc.vec[c], r);
        u.v[i] = u.v[i] + (r + alpha * kf[l.a * ms + i]);
      }
    }
    return u;
  }
};

// ---------------------------------------------------------------- linearisation
// row = one (problem, step) pair; lane a = member a
using LinC = rowsys::LinC<Par>;

template <int SYS, bool CEN>
__global__ __launch_bounds__(TPB) void linearize_kernel(LinC a) {
  constexpr int ns = state_dim(SYS), ms = control_dim(SYS);
  const long long g = rowsys::row_index();
  if (g >= a.batch * a.nuse) return;
  const Lane l = FleetRow<SYS>::lane_of(a.P);
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

template <int SYS>
int launch_linearize(FleetRow<SYS>, const LinC& a, hipStream_t st) {
  const dim3 grid(rowsys::row_grid(a.batch * (long long)a.nuse));
  if (a.central) hipLaunchKernelGGL((linearize_kernel<SYS, true>), grid, dim3(TPB), 0, st, a);
  else hipLaunchKernelGGL((linearize_kernel<SYS, false>), grid, dim3(TPB), 0, st, a);
  return set_hip_status(hipGetLastError());
}

static int params_of(const hop_fleet_params* q, Par* P) {
  if (!q) return set_error(HOP_E_ARG, "null fleet parameters");
  if (q->system < 0 || q->system >= kNumSystems)
    return set_error(HOP_E_ARG, "fleet: unknown system (0..4)");
  if (q->count < 1) return set_error(HOP_E_SIZE, "fleet: count must be >= 1");
  if (!shape_ok(q->system, q->count))
    return set_error(HOP_E_SIZE, "fleet: n must be <= 31 and m <= 16");
  if (!(q->dt > 0.0)) return set_error(HOP_E_ARG, "fleet: dt must be positive");
  *P = Par{q->system, q->count, q->dt};
  return HOP_OK;
}

// f(FleetRow<system>{}, P) for the validated parameters: every entry's first step
template <class F>
int with_fleet(const hop_fleet_params* q, F&& f) {
  Par P;
  if (int rc = params_of(q, &P)) return rc;
  switch (P.sys) {
    case kDI: return f(FleetRow<kDI>{}, P);
    case kCartpole: return f(FleetRow<kCartpole>{}, P);
    case kQuadrotor: return f(FleetRow<kQuadrotor>{}, P);
    case kPointmass: return f(FleetRow<kPointmass>{}, P);
    default: return f(FleetRow<kSegway>{}, P);
  }
}

}  // namespace fleet
}  // namespace hop

// the proximity cost: FleetProxRow<SYS> and the Taylor kernel (hop_fleet_proximity.h)
#include "../../include/hop_fleet_proximity.h"
#include "fleet_proximity.hpp"

// ---------------------------------------------------------------- C entries
namespace rowsys = hop::rowsys;
using hop::fleet::Par;
using hop::fleet::ProxPar;
using hop::fleet::with_fleet;
using hop::fleet::with_fleet_prox;

extern "C" {

int hop_fleet_dynamics_f64(const hop_fleet_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream) {
  return with_fleet(params, [&](auto s, const Par& P) {
    return rowsys::dynamics_entry<decltype(s)>(P, X, x_stride, U, u_stride, count, Xn, xn_stride,
                                               stream);
  });
}

int hop_fleet_rollout_f64(const hop_fleet_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream) {
  return with_fleet(params, [&](auto s, const Par& P) {
    return rowsys::rollout_entry<decltype(s)>(P, x0, x0_batch_stride, U, batch, N,
                                              max_state_norm, X, stream);
  });
}

int hop_fleet_linearize_f64(const hop_fleet_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream) {
  return with_fleet(params, [&](auto s, const Par& P) {
    if (int rc = rowsys::linearize_checks(X, U, batch, n_alloc, n_use, central, A, Bm,
                                          rowsys::kMaxRows))  // one row per (problem, step)
      return rc < 0 ? rc : (int)HOP_OK;
    const hop::fleet::LinC a{P,     central, epsx,  epsu, relx, relu,  X, U,
                             batch, n_alloc, n_use, A,    Bm,   a_res, Fx};
    return hop::fleet::launch_linearize(s, a, (hipStream_t)stream);
  });
}

int hop_fleet_cost_true_f64(const hop_fleet_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, uint32_t wrap_mask, int64_t batch,
                            int32_t N, double* J, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_fleet(params, [&](auto s, const Par& P) {
    return rowsys::cost_entry<decltype(s)>(P, X, U, T_star, cost, batch, N, J, stream);
  });
}

size_t hop_fleet_forward_workspace_bytes(const hop_fleet_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha) {
  if (!params || !hop::fleet::shape_ok(params->system, params->count)) return 0;
  return rowsys::workspace_bytes(params->count * hop::dyn::state_dim(params->system),
                                 params->count * hop::dyn::control_dim(params->system), batch, N,
                                 n_alpha);
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
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_fleet(params, [&](auto s, const Par& P) {
    return rowsys::linesearch_entry<decltype(s)>(P, X, U, cost, T_star, active, K, k, alphas,
                                                 n_alpha, batch, N, workspace, workspace_bytes,
                                                 X_new, U_new, J, J_old, accepted, stream);
  });
}

// ---- include/hop_fleet_proximity.h
int hop_fleet_proximity_taylor_f64(const hop_fleet_params* params,
                                   const hop_fleet_proximity* prox, const double* X,
                                   int64_t x_stride, int64_t count, double* c, double* cx,
                                   double* cxx, void* stream) {
  return with_fleet_prox(params, prox, [&](auto s, const ProxPar& P) {
    return hop::fleet::taylor_entry<hop::fleet::sys_of<typename decltype(s)::Base>::value>(
        P, X, x_stride, count, c, cx, cxx, stream);
  });
}

int hop_fleet_prox_cost_true_f64(const hop_fleet_params* params, const double* X,
                                 const double* U, const int32_t* T_star, const double* xg,
                                 int64_t xg_batch_stride, const double* u_ref,
                                 int64_t u_ref_batch_stride, const double* Q, const double* R,
                                 const double* Qf, const double* w, int64_t w_batch_stride,
                                 uint32_t wrap_mask, const hop_fleet_proximity* prox,
                                 int64_t batch, int32_t N, double* J, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_fleet_prox(params, prox, [&](auto s, const ProxPar& P) {
    return rowsys::cost_entry<decltype(s)>(P, X, U, T_star, cost, batch, N, J, stream);
  });
}

int hop_fleet_prox_forward_linesearch_f64(
    const hop_fleet_params* params, const double* X, const double* U, const double* xg,
    int64_t xg_batch_stride, const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
    const double* R, const double* Qf, const double* w, int64_t w_batch_stride,
    uint32_t wrap_mask, const hop_fleet_proximity* prox, const int32_t* T_star,
    const int32_t* active, const double* K, const double* k, const double* alphas,
    int32_t n_alpha, int64_t batch, int32_t N, void* workspace, size_t workspace_bytes,
    double* X_new, double* U_new, double* J, double* J_old, int32_t* accepted, void* stream) {
  const rowsys::CostC cost{xg, xg_batch_stride, u_ref, u_ref_batch_stride, Q, R, Qf, w,
                           w_batch_stride, wrap_mask};
  return with_fleet_prox(params, prox, [&](auto s, const ProxPar& P) {
    return rowsys::linesearch_entry<decltype(s)>(P, X, U, cost, T_star, active, K, k, alphas,
                                                 n_alpha, batch, N, workspace, workspace_bytes,
                                                 X_new, U_new, J, J_old, accepted, stream);
  });
}

}  // extern "C"
