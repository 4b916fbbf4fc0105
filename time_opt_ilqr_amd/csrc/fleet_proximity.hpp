// The proximity cost of a fleet (include/hop_fleet_proximity.h): Gaussian bumps between
// every member and the rows of an obstacle table, and between every pair of members.
// Included by fleet.hip after FleetRow<SYS>; two pieces:
//
// FleetProxRow<SYS>, the proximity variant of the row policy.  It is FleetRow<SYS> with a
// Par that carries the cost, an Lds that adds the staged table, and a stage_inc that adds
// c(x_k) after the plain increment (solver.py:96-99: acc += (q + r) + w, then acc +=
// c_extra).  Lane a publishes its pd positions in the row's exchange vector (the wave_sync
// pairs of half_quad_row), sums its bumps against the table and against the members after
// it, and the row total is one lane_sum<16>: the same bits on every lane.  It goes through
// rowsys::cost_entry / linesearch_entry unchanged.  A cost with no term skips all of it,
// so such a call is the plain fleet's bit for bit.
//
// taylor_kernel<SYS>: c, cx and cxx at one stacked state per 16-lane row.  Lane a forms the
// pair coefficients c_ab / r^2 for b > a once and parks them in LDS (a triangle of 120);
// every lane then sums its own gradient and diagonal block from them, and the n x n tile is
// written in row order by the row's 16 lanes, 128 contiguous bytes per store.  An
// off-diagonal entry is -(k (d_i d_j)) with d = p_a - p_b: the transposed entry forms
// (-d_j)(-d_i), the same bits, so cxx is symmetric bit for bit; a diagonal block sums
// k (d_i d_j) in one order for (i, j) and (j, i).
#pragma once

namespace hop {
namespace fleet {

constexpr int kMaxObs = 16;  // HOP_FLEET_MAX_OBSTACLES
constexpr int kMaxPd = 3;
constexpr int kObsLds = kMaxObs * (kMaxPd + 2);
// position entries of a member: the leading entries of its state
HOP_HD constexpr int pos_dim(int sys) { return sys == kQuadrotor ? 3 : sys == kPointmass ? 2 : 1; }

struct Prox {
  const double* obs;  // device, [n_obs][pd + 2]
  int n_obs;
  double sep_r, sep_w;
};
struct ProxPar : Par {
  Prox x;
};

// w exp(-|d|^2 / (2 r^2))
template <int PD>
__device__ __forceinline__ double bump(const double (&d)[PD], double r, double w) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < PD; ++i) s = fma(d[i], d[i], s);
  return w * exp(-s / (2.0 * r * r));
}

// all threads of the workgroup: the table into LDS (the caller's barrier follows)
template <int PD>
__device__ __forceinline__ void stage_obstacles(const Prox& x, double* obs) {
  for (int e = threadIdx.x; e < x.n_obs * (PD + 2); e += rowsys::TPB) obs[e] = x.obs[e];
}

// the lane's share of the row's cost: its bumps against the table and against the members
// after it.  pos: the row's published positions [count][PD].
template <int PD>
__device__ __forceinline__ double lane_bumps(const double (&p)[PD], const Lane& l, int count,
                                             const double* obs, int n_obs, double sep_r,
                                             double sep_w, const double* pos) {
  double part = 0.0;
  if (l.live) {
    for (int j = 0; j < n_obs; ++j) {
      const double* o = obs + j * (PD + 2);
      if (o[PD + 1] == 0.0) continue;
      double d[PD];
#pragma unroll
      for (int i = 0; i < PD; ++i) d[i] = p[i] - o[i];
      part += bump<PD>(d, o[PD], o[PD + 1]);
    }
    if (sep_w != 0.0)
      for (int b = l.a + 1; b < count; ++b) {
        double d[PD];
#pragma unroll
        for (int i = 0; i < PD; ++i) d[i] = p[i] - pos[b * PD + i];
        part += bump<PD>(d, sep_r, sep_w);
      }
  }
  return part;
}

template <int SYS>
struct FleetProxRow : FleetRow<SYS> {
  using Base = FleetRow<SYS>;
  using Par = ProxPar;
  using Lane = fleet::Lane;
  using typename Base::Input;
  using typename Base::State;
  static constexpr int pd = pos_dim(SYS);

  struct alignas(16) Lds {
    typename Base::Lds base;
    double obs[kObsLds];
  };
  HOP_ROWFN bool stage(const CostC& c, const Par& P, Lds& lds) {
    stage_obstacles<pd>(P.x, lds.obs);
    return Base::stage(c, P, lds.base);  // ends in the workgroup's barrier
  }

  struct RowCost : Base::RowCost {
    const double* obs;
    int n_obs, count;
    double sep_r, sep_w;
    bool any;  // the cost has a term
  };
  HOP_ROWFN RowCost row_cost_of(const CostC& c, const Par& P, const Lane& l, long long b,
                                Lds& lds, bool fast) {
    RowCost r;
    static_cast<typename Base::RowCost&>(r) = Base::row_cost_of(c, P, l, b, lds.base, fast);
    r.obs = lds.obs, r.n_obs = P.x.n_obs, r.count = P.count;
    r.sep_r = P.x.sep_r, r.sep_w = P.x.sep_w;
    r.any = P.x.n_obs > 0 || (P.x.sep_w != 0.0 && P.count > 1);
    return r;
  }

  // c(x) of the row's stacked state, the same bits on every lane
  HOP_ROWFN double prox_cost(const RowCost& rc, const Lane& l, const State& s) {
    double p[pd];
#pragma unroll
    for (int i = 0; i < pd; ++i) p[i] = s.v[i];
    wave_sync();  // the vector's readers of the step before are done
    store_slice<pd>(rc.vec, l, p);
    wave_sync();
    return lane_sum<16>(
        lane_bumps<pd>(p, l, rc.count, rc.obs, rc.n_obs, rc.sep_r, rc.sep_w, rc.vec));
  }

  HOP_ROWFN bool stage_inc(const RowCost& rc, const Lane& l, const State& s, const Input& u,
                           double& acc) {
    const bool ok = Base::stage_inc(rc, l, s, u, acc);
    if (rc.any) acc += prox_cost(rc, l, s);
    return ok;
  }
};

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
struct alignas(16) TaylorLds {
  double obs[kObsLds];
  double pos[kRows][16 * kMaxPd];            // the rows' positions [count][pd]
  double kg[kRows][kTri];                    // c_ab / r^2 of the pairs
  double diag[kRows][16 * kMaxPd * kMaxPd];  // the members' diagonal blocks [count][pd][pd]
};

template <int SYS>
__global__ __launch_bounds__(TPB) void taylor_kernel(TaylorC a) {
  constexpr int ns = state_dim(SYS), pd = pos_dim(SYS);
  __shared__ TaylorLds lds;
  const Prox x = a.P.x;
  stage_obstacles<pd>(x, lds.obs);
  __syncthreads();
  const long long r = rowsys::row_index();
  if (r >= a.count) return;
  const Lane l = FleetRow<SYS>::lane_of(a.P);
  const int cnt = a.P.count, n = cnt * ns, rw = threadIdx.x >> 4;
  double* pos = lds.pos[rw];
  double* kg = lds.kg[rw];
  double* diag = lds.diag[rw];
  const bool sep = x.sep_w != 0.0 && cnt > 1;
  const double ir2s = sep ? 1.0 / (x.sep_r * x.sep_r) : 0.0;

  double p[pd], g[pd], H[pd * pd];
#pragma unroll
  for (int i = 0; i < pd; ++i) {
    p[i] = l.live ? a.X[r * a.x_stride + l.a * ns + i] : 0.0;
    g[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < pd * pd; ++i) H[i] = 0.0;
  store_slice<pd>(pos, l, p);
  wave_sync();

  double part = 0.0;
  if (l.live) {
    for (int j = 0; j < x.n_obs; ++j) {
      const double* o = lds.obs + j * (pd + 2);
      if (o[pd + 1] == 0.0) continue;
      double d[pd];
#pragma unroll
      for (int i = 0; i < pd; ++i) d[i] = p[i] - o[i];
      const double ci = bump<pd>(d, o[pd], o[pd + 1]);
      const double ir2 = 1.0 / (o[pd] * o[pd]);
      const double k2 = ci * ir2, k4 = k2 * ir2;
      part += ci;
#pragma unroll
      for (int i = 0; i < pd; ++i) {
        g[i] = fma(-k2, d[i], g[i]);
#pragma unroll
        for (int jj = 0; jj < pd; ++jj) H[i * pd + jj] = fma(k4, d[i] * d[jj], H[i * pd + jj]);
      }
    }
    if (sep)  // the pairs' coefficients, once per row: lane a forms those of b > a
      for (int b = l.a + 1; b < cnt; ++b) {
        double d[pd];
#pragma unroll
        for (int i = 0; i < pd; ++i) d[i] = p[i] - pos[b * pd + i];
        const double ci = bump<pd>(d, x.sep_r, x.sep_w);
        part += ci;
        kg[tri(l.a, b)] = ci * ir2s;
      }
  }
  wave_sync();
  if (l.live && sep)
    for (int b = 0; b < cnt; ++b) {
      if (b == l.a) continue;
      const double k2 = kg[b < l.a ? tri(b, l.a) : tri(l.a, b)], k4 = k2 * ir2s;
      double d[pd];
#pragma unroll
      for (int i = 0; i < pd; ++i) d[i] = p[i] - pos[b * pd + i];
#pragma unroll
      for (int i = 0; i < pd; ++i) {
        g[i] = fma(-k2, d[i], g[i]);
#pragma unroll
        for (int jj = 0; jj < pd; ++jj) H[i * pd + jj] = fma(k4, d[i] * d[jj], H[i * pd + jj]);
      }
    }
  const double c = lane_sum<16>(part);
  if (a.c && l.a == 0) a.c[r] = c;
  if (a.cx && l.live) {
    double* o = a.cx + r * n + l.a * ns;
#pragma unroll
    for (int i = 0; i < ns; ++i) o[i] = i < pd ? g[i < pd ? i : 0] : 0.0;
  }
  if (!a.cxx) return;
  if (l.live) {
#pragma unroll
    for (int i = 0; i < pd * pd; ++i) diag[l.a * pd * pd + i] = H[i];
  }
  wave_sync();
  // the tile in row order: entry e = i n + j on lane e mod 16
  double* out = a.cxx + r * (long long)n * n;
  int i = 0, j = l.a;
  while (j >= n) j -= n, ++i;
  while (i < n) {
    const int ai = i / ns, ii = i - ai * ns, aj = j / ns, jj = j - aj * ns;
    double v = 0.0;
    if (ii < pd && jj < pd) {
      if (ai == aj) {
        v = diag[ai * pd * pd + ii * pd + jj];
      } else if (sep) {
        const double k4 = kg[ai < aj ? tri(ai, aj) : tri(aj, ai)] * ir2s;
        const double di = pos[ai * pd + ii] - pos[aj * pd + ii];
        const double dj = pos[ai * pd + jj] - pos[aj * pd + jj];
        v = -(k4 * (di * dj));
      }
    }
    out[i * n + j] = v;
    j += 16;
    while (j >= n) j -= n, ++i;
  }
}

// the cost's host checks (include/hop_fleet_proximity.h)
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
  *x = Prox{q->obstacles, q->n_obs, q->sep_radius, q->sep_weight};
  return HOP_OK;
}

template <class Row>
struct sys_of;
template <int SYS>
struct sys_of<FleetRow<SYS>> {
  static constexpr int value = SYS;
};

// f(FleetProxRow<system>{}, P) for the validated fleet and cost
template <class F>
int with_fleet_prox(const hop_fleet_params* q, const hop_fleet_proximity* prox, F&& f) {
  return with_fleet(q, [&](auto s, const Par& P) {
    ProxPar PP;
    static_cast<Par&>(PP) = P;
    if (int rc = prox_of(prox, &PP.x)) return rc;
    constexpr int sys = sys_of<decltype(s)>::value;
    return f(FleetProxRow<sys>{}, PP);
  });
}

template <int SYS>
int taylor_entry(const ProxPar& P, const double* X, int64_t x_stride, int64_t count, double* c,
                 double* cx, double* cxx, void* stream) {
  if (count < 0) return set_error(HOP_E_ARG, "count < 0");
  if (x_stride < P.count * state_dim(SYS)) return set_error(HOP_E_ARG, "row stride too small");
  if (count == 0 || (!c && !cx && !cxx)) return HOP_OK;
  if (!X) return set_error(HOP_E_ARG, "null input pointer");
  if (!rowsys::rows_fit(count)) return set_error(HOP_E_SIZE, "count too large for one launch");
  const TaylorC a{P, X, x_stride, count, c, cx, cxx};
  hipLaunchKernelGGL(taylor_kernel<SYS>, dim3(rowsys::row_grid(count)), dim3(TPB), 0,
                     (hipStream_t)stream, a);
  return set_hip_status(hipGetLastError());
}

}  // namespace fleet
}  // namespace hop
