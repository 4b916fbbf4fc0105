// The proximity cost of a team (include/hop_mixed_proximity.h): the fleets' Gaussian bumps
// (fleet_proximity.hpp) between members whose positions differ in dimension.  Positions
// live in a workspace of dimension D, the largest pd among the members; member a's
// workspace position is its pd_a leading state entries padded with zeros to D, and a
// gradient or second-order block is restricted to the coordinates a member has.
// Included by team.hip after TeamRow<NSMAX, MSMAX>; two pieces:
//
// TeamProxRow<NSMAX, MSMAX>, the proximity variant of the row policy.  It is TeamRow with a
// Par that carries the cost, an Lds that adds the staged table and a position slab of its
// own (the row's exchange vector holds n doubles and 3 count can exceed it), and a
// stage_inc that adds c(x_k) after the plain increment (solver.py:96-99).  A lane decodes
// its pd from its kind, publishes its padded position, sums its bumps against the table
// and against the members after it, and the row total is one lane_sum<16>: the same bits on
// every lane.  It goes through rowsys::cost_entry / linesearch_entry unchanged.  A cost
// with no term skips all of it, so such a call is the plain team's bit for bit.  The order
// of every sum is FleetProxRow's -- obstacle rows ascending, then b = a + 1 ..., |d|^2 by
// ascending fma, a padded coordinate adding fma(0, 0, s) = s -- so a team of equal members
// gives the fleet's bits.
//
// taylor_kernel<DM>: c, cx and cxx at one stacked state per 16-lane row, the Shape by value.
// Lane a parks the pair coefficients c_ab / r^2 for b > a in LDS (a triangle of 120), every
// lane sums its own gradient and D x D diagonal block from them, and the n x n tile is
// written in row order by the row's 16 lanes, 128 contiguous bytes per store, the blocks
// rectangular pd_a x pd_b at (xo_a, xo_b).  An off-diagonal entry is -(k (d_i d_j)) with
// d = P_a - P_b: the transposed entry forms (-d_j)(-d_i), the same bits, so cxx is
// symmetric bit for bit; a diagonal block sums k (d_i d_j) in one order for (i, j) and
// (j, i).
#pragma once

namespace hop {
namespace team {

constexpr int kMaxObs = 16;  // HOP_FLEET_MAX_OBSTACLES
constexpr int kMaxPd = 3;
constexpr int kObsLds = kMaxObs * (kMaxPd + 2);
// position entries of a member: the leading entries of its state (fleet::pos_dim's rule)
HOP_HD constexpr int pos_dim(int sys) { return sys == kQuadrotor ? 3 : sys == kPointmass ? 2 : 1; }

struct Prox {
  const double* obs;  // device, [n_obs][D + 2]
  int n_obs, D;       // D: the workspace dimension, the largest pd among the members
  double sep_r, sep_w;
};
struct ProxPar : Par {
  Prox x;
};

// w exp(-|d|^2 / (2 r^2)); the entries of d at and above D are zeros and leave s as it is
template <int DM>
__device__ __forceinline__ double bump(const double (&d)[DM], double r, double w) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < DM; ++i) s = fma(d[i], d[i], s);
  return w * exp(-s / (2.0 * r * r));
}

// all threads of the workgroup: the table into LDS (the caller's barrier follows)
__device__ __forceinline__ void stage_obstacles(const Prox& x, double* obs) {
  for (int e = threadIdx.x; e < x.n_obs * (x.D + 2); e += TPB) obs[e] = x.obs[e];
}

// the lane's padded position: its pd leading state entries, zeros up to DM
template <int DM, int K>
__device__ __forceinline__ void position_of(const Lane& l, const double (&v)[K], double (&p)[DM]) {
  const int pd = pos_dim(l.kind);
#pragma unroll
  for (int i = 0; i < DM; ++i) p[i] = l.live && i < pd ? v[i] : 0.0;
}

// the lane's share of the row's cost: its bumps against the table, then against the members
// after it, in one loop (one expansion of exp): item j < n_obs is obstacle row j, item
// n_obs + i is member a + 1 + i.  pos: the row's published positions [count][DM].
template <int DM>
__device__ __forceinline__ double lane_bumps(const double (&p)[DM], const Lane& l, int count,
                                             const double* obs, int n_obs, int D, double sep_r,
                                             double sep_w, const double* pos) {
  double part = 0.0;
  if (l.live) {
    const int items = n_obs + (sep_w != 0.0 ? count - l.a - 1 : 0);
    for (int j = 0; j < items; ++j) {
      const bool ob = j < n_obs;
      const double* q = ob ? obs + j * (D + 2) : pos + (l.a + 1 + j - n_obs) * DM;
      const double r = ob ? q[D] : sep_r, w = ob ? q[D + 1] : sep_w;
      if (w == 0.0) continue;
      double d[DM];
#pragma unroll
      for (int i = 0; i < DM; ++i) d[i] = !ob || i < D ? p[i] - q[i] : 0.0;
      part += bump<DM>(d, r, w);
    }
  }
  return part;
}

template <int NSMAX, int MSMAX>
struct TeamProxRow : TeamRow<NSMAX, MSMAX> {
  using Base = TeamRow<NSMAX, MSMAX>;
  using Par = ProxPar;
  using Lane = team::Lane;
  using typename Base::Input;
  using typename Base::State;
  static constexpr int DM = Base::kQuad ? 3 : 2;  // the largest D of the instantiation

  // the cost's scalars sit in LDS beside the table, so that a row holds none of them in
  // registers along the horizon
  struct alignas(16) Lds {
    typename Base::Lds base;
    double obs[kObsLds];
    double pos[kRows * 16 * DM];  // the rows' positions [count][DM]
    double sep[2];                // separation radius, weight
    int dims[2];                  // n_obs, D
  };
  HOP_ROWFN bool stage(const CostC& c, const Par& P, Lds& lds) {
    stage_obstacles(P.x, lds.obs);
    if (threadIdx.x == 0) {
      lds.sep[0] = P.x.sep_r, lds.sep[1] = P.x.sep_w;
      lds.dims[0] = P.x.n_obs, lds.dims[1] = P.x.D;
    }
    return Base::stage(c, P, lds.base);  // ends in the workgroup's barrier
  }

  struct RowCost : Base::RowCost {
    const Lds* lds;
    double* pos;  // the row's slab
    int count;    // 0: the cost has no term
  };
  HOP_ROWFN RowCost row_cost_of(const CostC& c, const Par& P, const Lane& l, long long b,
                                Lds& lds, bool fast) {
    RowCost r;
    static_cast<typename Base::RowCost&>(r) = Base::row_cost_of(c, P, l, b, lds.base, fast);
    r.lds = &lds, r.pos = lds.pos + (threadIdx.x >> 4) * 16 * DM;
    const bool any = P.x.n_obs > 0 || (P.x.sep_w != 0.0 && P.s.count > 1);
    r.count = any ? P.s.count : 0;
    return r;
  }

  // c(x) of the row's stacked state, the same bits on every lane
  HOP_ROWFN double prox_cost(const RowCost& rc, const Lane& l, const State& s) {
    double p[DM];
    position_of<DM>(l, s.v, p);
    wave_sync();  // the slab's readers of the step before are done
    if (l.live) {
#pragma unroll
      for (int i = 0; i < DM; ++i) rc.pos[l.a * DM + i] = p[i];
    }
    wave_sync();
    const Lds& L = *rc.lds;
    return lane_sum<16>(lane_bumps<DM>(p, l, rc.count, L.obs, L.dims[0], L.dims[1], L.sep[0],
                                       L.sep[1], rc.pos));
  }

  HOP_ROWFN bool stage_inc(const RowCost& rc, const Lane& l, const State& s, const Input& u,
                           double& acc) {
    const bool ok = Base::stage_inc(rc, l, s, u, acc);
    if (rc.count) acc += prox_cost(rc, l, s);
    return ok;
  }
};

}  // namespace team

// rowsys::row_cost_true of the two proximity policies, inlined by force: left to its own
// judgement the compiler keeps the <12, 4> one as a call in the line-search kernel and passes
// RowCost and Lane through scratch.  The body is row_system.hpp's.
namespace rowsys {
template <class Sys>
__device__ __forceinline__ double prox_row_cost_true(const typename Sys::RowCost& rc,
                                                     const typename Sys::Par& P,
                                                     const typename Sys::Lane& l, const double* X,
                                                     const double* U, int T) {
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
template <>
__device__ __forceinline__ double row_cost_true<team::TeamProxRow<12, 4>>(
    const team::TeamProxRow<12, 4>::RowCost& rc, const team::ProxPar& P, const team::Lane& l,
    const double* X, const double* U, int T) {
  return prox_row_cost_true<team::TeamProxRow<12, 4>>(rc, P, l, X, U, T);
}
template <>
__device__ __forceinline__ double row_cost_true<team::TeamProxRow<4, 2>>(
    const team::TeamProxRow<4, 2>::RowCost& rc, const team::ProxPar& P, const team::Lane& l,
    const double* X, const double* U, int T) {
  return prox_row_cost_true<team::TeamProxRow<4, 2>>(rc, P, l, X, U, T);
}
}  // namespace rowsys

namespace team {

// ---------------------------------------------------------------- Taylor terms
constexpr int kTri = 120;  // pairs a < b of 16 members
__device__ __forceinline__ int tri(int lo, int hi) {
  return lo * 16 - (lo * (lo + 1)) / 2 + (hi - lo - 1);
}

struct TaylorC {
  ProxPar P;
  const double* X;
  long long x_stride, count;
  double* c; double* cx; double* cxx;
};
template <int DM>
struct alignas(16) TaylorLds {
  double obs[kObsLds];
  double pos[kRows][16 * DM];       // the rows' positions [count][DM]
  double kg[kRows][kTri];           // c_ab / r^2 of the pairs
  double diag[kRows][16 * DM * DM]; // the members' diagonal blocks [count][DM][DM]
  int who[kVec];                    // state index -> member << 8 | pd << 4 | entry
};

template <int DM>
__global__ __launch_bounds__(TPB) void taylor_kernel(TaylorC a) {
  constexpr int NSM = DM == 3 ? state_dim(kQuadrotor) : 4;  // TeamRow's NSMAX
  __shared__ TaylorLds<DM> lds;
  const Prox x = a.P.x;
  const Shape& sh = a.P.s;
  stage_obstacles(x, lds.obs);
  Lane l;
  l.a = rowsys::row_lane();
  l.live = l.a < sh.count;
  l.kind = l.live ? kind_of(sh, l.a) : 0;
  l.xo = l.live ? xo_of(sh, l.a) : 0;
  l.ns = l.live ? state_dim(l.kind) : 0;
  l.uo = l.ms = 0;
  const int pd = pos_dim(l.kind);
  if (threadIdx.x < 16 && l.live) {  // the workgroup's first row always exists
#pragma unroll
    for (int i = 0; i < NSM; ++i)
      if (i < l.ns) lds.who[l.xo + i] = (l.a << 8) | (pd << 4) | i;
  }
  __syncthreads();
  const long long r = rowsys::row_index();
  if (r >= a.count) return;
  const int cnt = sh.count, n = sh.n, D = x.D, rw = threadIdx.x >> 4;
  double* pos = lds.pos[rw];
  double* kg = lds.kg[rw];
  double* diag = lds.diag[rw];
  const bool sep = x.sep_w != 0.0 && cnt > 1;
  const double ir2s = sep ? 1.0 / (x.sep_r * x.sep_r) : 0.0;

  double p[DM], g[DM], H[DM * DM];
#pragma unroll
  for (int i = 0; i < DM; ++i) {
    p[i] = l.live && i < pd ? a.X[r * a.x_stride + l.xo + i] : 0.0;
    g[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < DM * DM; ++i) H[i] = 0.0;
  if (l.live) {
#pragma unroll
    for (int i = 0; i < DM; ++i) pos[l.a * DM + i] = p[i];
  }
  wave_sync();

  double part = 0.0;
  if (l.live) {
    for (int j = 0; j < x.n_obs; ++j) {
      const double* o = lds.obs + j * (D + 2);
      if (o[D + 1] == 0.0) continue;
      double d[DM];
#pragma unroll
      for (int i = 0; i < DM; ++i) d[i] = i < D ? p[i] - o[i] : 0.0;
      const double ci = bump<DM>(d, o[D], o[D + 1]);
      const double ir2 = 1.0 / (o[D] * o[D]);
      const double k2 = ci * ir2, k4 = k2 * ir2;
      part += ci;
#pragma unroll
      for (int i = 0; i < DM; ++i) {
        g[i] = fma(-k2, d[i], g[i]);
#pragma unroll
        for (int jj = 0; jj < DM; ++jj) H[i * DM + jj] = fma(k4, d[i] * d[jj], H[i * DM + jj]);
      }
    }
    if (sep)  // the pairs' coefficients, once per row: lane a forms those of b > a
      for (int b = l.a + 1; b < cnt; ++b) {
        double d[DM];
#pragma unroll
        for (int i = 0; i < DM; ++i) d[i] = p[i] - pos[b * DM + i];
        const double ci = bump<DM>(d, x.sep_r, x.sep_w);
        part += ci;
        kg[tri(l.a, b)] = ci * ir2s;
      }
  }
  wave_sync();
  if (l.live && sep)
    for (int b = 0; b < cnt; ++b) {
      if (b == l.a) continue;
      const double k2 = kg[b < l.a ? tri(b, l.a) : tri(l.a, b)], k4 = k2 * ir2s;
      double d[DM];
#pragma unroll
      for (int i = 0; i < DM; ++i) d[i] = p[i] - pos[b * DM + i];
#pragma unroll
      for (int i = 0; i < DM; ++i) {
        g[i] = fma(-k2, d[i], g[i]);
#pragma unroll
        for (int jj = 0; jj < DM; ++jj) H[i * DM + jj] = fma(k4, d[i] * d[jj], H[i * DM + jj]);
      }
    }
  const double c = lane_sum<16>(part);
  if (a.c && l.a == 0) a.c[r] = c;
  if (a.cx && l.live) {
    double* o = a.cx + r * n + l.xo;
#pragma unroll
    for (int i = 0; i < NSM; ++i)
      if (i < l.ns) o[i] = i < pd ? g[i < DM ? i : 0] : 0.0;
  }
  if (!a.cxx) return;
  if (l.live) {
#pragma unroll
    for (int i = 0; i < DM * DM; ++i) diag[l.a * DM * DM + i] = H[i];
  }
  wave_sync();
  // the tile in row order: entry e = i n + j on lane e mod 16
  double* out = a.cxx + r * (long long)n * n;
  int i = 0, j = l.a;
  while (j >= n) j -= n, ++i;
  while (i < n) {
    const int wi = lds.who[i], wj = lds.who[j];
    const int ai = wi >> 8, ii = wi & 15, aj = wj >> 8, jj = wj & 15;
    double v = 0.0;
    if (ii < ((wi >> 4) & 15) && jj < ((wj >> 4) & 15)) {
      if (ai == aj) {
        v = diag[ai * DM * DM + ii * DM + jj];
      } else if (sep) {
        const double k4 = kg[ai < aj ? tri(ai, aj) : tri(aj, ai)] * ir2s;
        const double di = pos[ai * DM + ii] - pos[aj * DM + ii];
        const double dj = pos[ai * DM + jj] - pos[aj * DM + jj];
        v = -(k4 * (di * dj));
      }
    }
    out[i * n + j] = v;
    j += 16;
    while (j >= n) j -= n, ++i;
  }
}

// the cost's host checks (include/hop_fleet_proximity.h's)
static int prox_of(const hop_fleet_proximity* q, Prox* x) {
  if (!q) return set_error(HOP_E_ARG, "null proximity parameters");
  if (q->n_obs < 0 || q->n_obs > kMaxObs)
    return set_error(HOP_E_ARG, "proximity: n_obs must be in [0, 16]");
  if (q->n_obs > 0 && !q->obstacles)
    return set_error(HOP_E_ARG, "proximity: null obstacle table with n_obs > 0");
  if (!(q->sep_weight >= 0.0) || !(q->sep_weight - q->sep_weight == 0.0))
    return set_error(HOP_E_ARG, "proximity: the separation weight must be finite and >= 0");
  if (q->sep_weight > 0.0 && !(q->sep_radius > 0.0 && q->sep_radius - q->sep_radius == 0.0))
    return set_error(HOP_E_ARG, "proximity: the separation radius must be finite and > 0");
  x->obs = q->obstacles, x->n_obs = q->n_obs;
  x->sep_r = q->sep_radius, x->sep_w = q->sep_weight;
  return HOP_OK;
}

// f(TeamProxRow<...>{}, P) for the validated composition and cost; dt is checked where the
// entry steps (step), else it is not read
template <class F>
int with_mixed_prox(int32_t members, const int32_t* system, bool step, double dt,
                    const hop_fleet_proximity* prox, F&& f) {
  ProxPar P;
  if (members >= 1 && members <= kMaxMembers && !system)
    return set_error(HOP_E_ARG, "team: null member list");
  switch (shape_of(members, system, &P.s)) {
    case 0: break;
    case 1: return set_error(HOP_E_SIZE, "team: count must be in [1, 15]");
    case 2: return set_error(HOP_E_ARG, "team: unknown member system (0..4)");
    default: return set_error(HOP_E_SIZE, "team: n must be <= 31 and m <= 16");
  }
  if (step && !(dt > 0.0)) return set_error(HOP_E_ARG, "team: dt must be positive");
  P.dt = step ? dt : 1.0;
  if (int rc = prox_of(prox, &P.x)) return rc;
  P.x.D = 1;
  for (int a = 0; a < members; ++a)
    if (pos_dim(system[a]) > P.x.D) P.x.D = pos_dim(system[a]);
  if (P.s.quad) return f(TeamProxRow<12, 4>{}, P);
  return f(TeamProxRow<4, 2>{}, P);
}

inline int taylor_entry(const ProxPar& P, const double* X, int64_t x_stride, int64_t count,
                        double* c, double* cx, double* cxx, void* stream) {
  if (count < 0) return set_error(HOP_E_ARG, "count < 0");
  if (x_stride < P.s.n) return set_error(HOP_E_ARG, "row stride too small");
  if (count == 0 || (!c && !cx && !cxx)) return HOP_OK;
  if (!X) return set_error(HOP_E_ARG, "null input pointer");
  if (!rowsys::rows_fit(count)) return set_error(HOP_E_SIZE, "count too large for one launch");
  const TaylorC a{P, X, x_stride, count, c, cx, cxx};
  const dim3 grid(rowsys::row_grid(count));
  if (P.s.quad)
    hipLaunchKernelGGL(taylor_kernel<3>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(taylor_kernel<2>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  return set_hip_status(hipGetLastError());
}

}  // namespace team
}  // namespace hop
