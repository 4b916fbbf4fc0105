// Wide Riccati backward passes (n <= 31, m <= 16, fp64), one problem per wave64 in the
// register layout of hop_wide_device.hpp; the passes and failure semantics of riccati.hip:
//   mode 0 = backward_pass_truncated           (solver.py:156-230)
//   mode 1 = value_expansions_and_gains_prefix (horizon_selection.py:97-212)
// n-sized matrices (Vxx, A, Qxx, ...) hold HR rows per half wave; m-row objects (Quu,
// Qux, K) hold 8 rows per half (m <= 16), so only the n-sized objects are wide.  A
// vector holds entry c on lane c (both halves).  A wave is one problem, so a failed
// problem simply stops: there is no workgroup barrier and no cross-problem state.
#include <math.h>

#include "hop_wide_device.hpp"
#include "hop_kernels.hpp"
#include "../../include/hop_wide.h"
#include "../../include/hop_wide_jcurve.h"

namespace hop {
namespace wide {

constexpr int MR = 8;  // rows per half of an m-row object

// zero outside rows x cols
template <int OR>
__device__ __forceinline__ void mask2(double (&x)[OR], const Ctx& w, int rows, int cols) {
#pragma unroll
  for (int i = 0; i < OR; ++i) x[i] = (w.h * OR + i < rows && w.c < cols) ? x[i] : 0.0;
}
// column c of a rows x cols row-major matrix, zero padded
template <int OR>
__device__ __forceinline__ void load_cols(const double* M, int rows, int cols, const Ctx& w,
                                          double (&x)[OR]) {
#pragma unroll
  for (int i = 0; i < OR; ++i) {
    const int r = w.h * OR + i;
    const bool in = r < rows && w.c < cols;
    const double v = M[in ? r * cols + w.c : 0];
    x[i] = in ? v : 0.0;
  }
}
// the transpose of a rows x cols row-major matrix: x[r] = M[c][r], zero padded
template <int OR>
__device__ __forceinline__ void load_rows(const double* M, int rows, int cols, const Ctx& w,
                                          double (&x)[OR]) {
#pragma unroll
  for (int i = 0; i < OR; ++i) {
    const int r = w.h * OR + i;
    const bool in = w.c < rows && r < cols;
    const double v = M[in ? w.c * cols + r : 0];
    x[i] = in ? v : 0.0;
  }
}
template <int OR>
__device__ __forceinline__ void store_cols(double* M, int rows, int cols, const Ctx& w,
                                           const double (&x)[OR]) {
#pragma unroll
  for (int i = 0; i < OR; ++i) {
    const int r = w.h * OR + i;
    if (r < rows && w.c < cols) M[r * cols + w.c] = x[i];
  }
}

// (M^T x)[c] = sum_r M[r][c] x[r]; x: entry c on lane c, zero past its length
template <int OR>
__device__ __forceinline__ double dot_col(const double (&M)[OR], double x, const Ctx& w) {
  if (w.h == 0) w.col[w.c] = x;
  wave_sync();
  double y = 0.0;
#pragma unroll
  for (int i = 0; i < OR; ++i) y = __builtin_fma(M[i], w.col[w.h * OR + i], y);
  y += __shfl_xor(y, 32);
  wave_sync();
  return y;
}
// sum over lanes c < 32 of half 0 (x is the same on both halves)
__device__ __forceinline__ double vec_sum(double x) {
  x += __shfl_xor(x, 16);
  x += __shfl_xor(x, 8);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 1);
  return x;
}
__device__ __forceinline__ bool any_lane(bool p) { return __any(p) != 0; }

// x <- 1/2 (x + x^T) through the left image.  put writes rows 0 .. 2 HR - 1 of the
// image and get_t reads row c on every lane: for HR < 16 the lanes c >= 2 HR read rows
// this put has not written (whatever the kernel before left in LDS), so only values
// from inside the block enter the registers and the padding stays exact zeros.
template <int HR>
__device__ __forceinline__ void symmetrize(double (&x)[HR], const Ctx& w) {
  put(w.L, x, w);
  wave_sync();
  double t[HR];
  get_t(w.L, t, w);
  wave_sync();
#pragma unroll
  for (int i = 0; i < HR; ++i) x[i] = live<HR>(w, i) ? 0.5 * (x[i] + t[i]) : 0.0;
}

// out (+)= X Y or X^T Y with explicit contraction count; x has XR rows per half, y YR,
// out OR (the n-sized objects HR, the m-row objects MR)
template <bool XT, int OR, int XR, int YR>
__device__ __forceinline__ void prod2(double (&out)[OR], const double (&x)[XR],
                                      const double (&y)[YR], int cnt, const Ctx& w) {
  if constexpr (XT) put(w.L, x, w);
  else put_t(w.L, x, w);
  put(w.Y, y, w);
  wave_sync();
  mul<false>(out, w.L, w.Y, cnt, w);
  wave_sync();
}

// utils.chol_solve's factorisation ladder on the m x m block r (symmetric): eps = 1e-9,
// x10 per failure, max_tries attempts, no LU slot.  r <- (r + eps I)^-1; false when
// every attempt failed (the reference raises LinAlgError).
__device__ __forceinline__ bool spd_inverse_nofallback(double (&r)[MR], const Ctx& wm,
                                                       int max_tries, unsigned& st) {
  double keep[MR];
#pragma unroll
  for (int i = 0; i < MR; ++i) keep[i] = r[i];
  double eps = 1e-9;
  int tries = 0;
  bool good = false;
#pragma unroll 1
  while (true) {
    bool ok = true;
    sweep_neg_inverse(r, eps, wm, ok);
    ++tries;
    good = ok;
    if (ok || tries >= max_tries) break;
    eps *= 10.0;
    st |= ST_JITTER;
#pragma unroll
    for (int i = 0; i < MR; ++i) r[i] = keep[i];
  }
#pragma unroll
  for (int i = 0; i < MR; ++i) r[i] = -r[i];
  return good;
}

// JC: the J-curve form (hop_bruteforce_jcurve_wide_f64, solver.py:293-358), on the mode-1
// step.  Wave g of the launch runs problem g / jc_tmax at horizon jc_tmax - g % jc_tmax,
// so a problem's horizons are adjacent and longest first and the re-reads of its A, B,
// X, U meet in the caches (riccati.hip's riccati_jcurve_kernel has that order per
// workgroup).  lm is the scalar lm_value, nothing of K, k, V is stored, V_0 and the status
// go to jc_J / jc_status[prob][L - 1], and the failure rules are the brute-force curve's.
// Every JC branch is a compile-time one: the single-pass instantiations compile to what
// they were without it.
template <int HR, int MODE, bool JC = false>
__global__ __launch_bounds__(64 * kWavesPerBlockW) void riccati_wide_kernel(RiccatiArgs<double> a) {
  __shared__ __attribute__((aligned(16))) double smem[kWavesPerBlockW * kLdsWave];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long wave = (long long)blockIdx.x * kWavesPerBlockW + wv;
  if (wave >= (JC ? a.batch * a.jc_tmax : a.batch)) return;  // wave-uniform
  const long long prob = JC ? wave / a.jc_tmax : wave;
  const int jl = JC ? a.jc_tmax - (int)(wave - prob * a.jc_tmax) : 0;
  const int n = a.n, m = a.m, NA = a.nalloc;
  Ctx w;
  w.L = smem + wv * kLdsWave;
  w.Y = w.L + kImg;
  w.col = w.Y + kImg;
  w.rinv = w.col + 32;
  w.bt = w.rinv + 16 * kRinvLd;
  w.c = lane & 31;
  w.h = lane >> 5;
  w.s = n;
  Ctx wm = w;  // the m x m solves
  wm.s = m;
  const int c = w.c;

  const long long nn = (long long)n * n, nm = (long long)n * m;
  const double* Ap = a.A + prob * NA * nn;
  const double* Bp = a.Bm + prob * NA * nm;
  const double* Xp = a.X + prob * (NA + 1) * n;
  const double* Up = a.U + prob * NA * m;
  const double* xgp = a.xg + prob * a.xg_bstride;
  const double* urp = a.u_ref + prob * a.uref_bstride;
  const double* Qp = a.Q + prob * a.q_bstride;
  const double* Rp = a.R + prob * a.r_bstride;
  const double* Qfp = a.Qf + prob * a.qf_bstride;
  const int L = JC ? jl : a.horizon[prob];
  const double lam0 = JC ? a.lm_value : a.lm[prob];

  // loop-invariant cost blocks: Q and R by columns and transposed
  double qcol[HR], qT[HR], rcol[MR], rT[MR];
  load_cols(Qp, n, n, w, qcol);
  load_rows(Qp, n, n, w, qT);
  load_cols(Rp, m, m, w, rcol);
  load_rows(Rp, m, m, w, rT);
  const double xg_c = (c < n) ? xgp[c < n ? c : 0] : 0.0;
  const double ur_c = (c < m) ? urp[c < m ? c : 0] : 0.0;
  const bool wrap_c = (c < n) && ((a.wrap_mask >> c) & 1u);

  unsigned st = 0;
  bool alive = L > 0 && L <= NA;
  if (!alive) st |= ST_FAIL;

  // terminal: Vxx = sym(Qf), Vx = Qf eT, V0 = 1/2 eT' Qf eT
  double Vxx[HR], vx = 0.0, v0 = 0.0;
  load_cols(Qfp, n, n, w, Vxx);
  {
    double qfT[HR];
    load_rows(Qfp, n, n, w, qfT);
    const int iT = alive ? L : 0;
    double eT = (c < n) ? Xp[(long long)iT * n + (c < n ? c : 0)] - xg_c : 0.0;
    if (wrap_c) eT = wrap_angle(eT);
    if (any_lane(!finite_val(eT))) {
      st |= ST_NONFINITE | ST_FAIL;
      alive = false;
    }
    vx = dot_col(qfT, eT, w);
    v0 = 0.5 * vec_sum((c < n) ? eT * vx : 0.0);
    symmetrize(Vxx, w);
    if (!JC && alive) {
      if (a.Vxx) store_cols(a.Vxx + (prob * (NA + 1) + L) * nn, n, n, w, Vxx);
      if (a.Vx && c < n && w.h == 0) a.Vx[prob * (NA + 1) * n + (long long)L * n + c] = vx;
      if (a.V0 && lane == 0) a.V0[prob * (NA + 1) + L] = v0;
    }
  }

#pragma unroll 1
  for (int i = (alive ? L : 0) - 1; i >= 0 && alive; --i) {
    double e = (c < n) ? Xp[(long long)i * n + (c < n ? c : 0)] - xg_c : 0.0;
    if (wrap_c) e = wrap_angle(e);
    const double du = (c < m) ? Up[(long long)i * m + (c < m ? c : 0)] - ur_c : 0.0;
    // the brute-force curve (solver.py:326-356) checks nothing itself: only its
    // chol_solve raises, so a non-finite e at t = 0 only feeds V_0 (inf / NaN in J)
    const bool e_ok = (JC && i == 0) || finite_val(e);
    const bool bad = any_lane(!(e_ok && finite_val(du)));

    // lx = Q e (+ cx), lu = R du, l0
    double lx = dot_col(qT, e, w);
    const double lu = dot_col(rT, du, w);
    double l0 = 0.5 * vec_sum((c < n) ? e * lx : 0.0) + 0.5 * vec_sum((c < m) ? du * lu : 0.0) +
                a.w_stage;
    double Qxx[HR];
#pragma unroll
    for (int r = 0; r < HR; ++r) Qxx[r] = qcol[r];
    if (a.qx_extra) lx += (c < n) ? a.qx_extra[(prob * NA + i) * n + (c < n ? c : 0)] : 0.0;
    if (a.c_extra) l0 += a.c_extra[prob * NA + i];
    if (a.qxx_extra) {
      double ex[HR];
      load_cols(a.qxx_extra + (prob * NA + i) * nn, n, n, w, ex);
#pragma unroll
      for (int r = 0; r < HR; ++r) Qxx[r] += ex[r];
      symmetrize(Qxx, w);
    }

    // Q-function assembly
    double acol[HR], bcol[HR];
    load_cols(Ap + (long long)i * nn, n, n, w, acol);
    load_cols(Bp + (long long)i * nm, n, m, w, bcol);
    const double qx = lx + dot_col(acol, vx, w);  // Qx = lx + A^T Vx
    const double qu = lu + dot_col(bcol, vx, w);  // Qu = lu + B^T Vx   (lanes < m)
    double Quu[MR], Qux[MR];
    {
      double VA[HR], VB[HR];
#pragma unroll
      for (int r = 0; r < HR; ++r) VA[r] = VB[r] = 0.0;
      prod2<false>(VA, Vxx, acol, n, w);   // Vxx A
      mask2(VA, w, n, n);
      prod2<false>(VB, Vxx, bcol, n, w);   // Vxx B          (lanes < m)
      mask2(VB, w, n, m);
      prod2<true>(Qxx, acol, VA, n, w);    // Qst + A^T Vxx A
      mask2(Qxx, w, n, n);
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        Quu[r] = rcol[r];
        Qux[r] = 0.0;
      }
      prod2<true>(Quu, bcol, VB, n, w);    // R + B^T Vxx B   (m x m)
      mask2(Quu, w, m, m);
      prod2<true>(Qux, bcol, VA, n, w);    // B^T Vxx A       (m x n)
      mask2(Qux, w, m, n);
    }

    // regularised solve: Quu_reg = sym(Quu) + lam I ; (Quu_reg + eps I)^-1
    double QuuT[MR];
    put(w.L, Quu, w);
    wave_sync();
    get_t(w.L, QuuT, w);
    wave_sync();
    double Qi[MR];
    bool solved = false;
    if constexpr (MODE == 0) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        Qi[r] = (w.h * MR + r < m && c < m)
                    ? 0.5 * (Quu[r] + QuuT[r]) + ((c == w.h * MR + r) ? lam0 : 0.0) : 0.0;
      // the reference first checks cholesky(Quu_reg) (no jitter), then solves with jitter
      bool ok0 = true;
      {
        double chk[MR];
#pragma unroll
        for (int r = 0; r < MR; ++r) chk[r] = Qi[r];
        sweep_neg_inverse(chk, 0.0, wm, ok0);
      }
      solved = spd_inverse_nofallback(Qi, wm, 8, st) && ok0;
    } else {
      double lam = lam0 > 1e-12 ? lam0 : 1e-12;
      int tries = 0;
#pragma unroll 1
      while (true) {
#pragma unroll
        for (int r = 0; r < MR; ++r)
          Qi[r] = (w.h * MR + r < m && c < m)
                      ? 0.5 * (Quu[r] + QuuT[r]) + ((c == w.h * MR + r) ? lam : 0.0) : 0.0;
        solved = spd_inverse_nofallback(Qi, wm, 8, st);
        ++tries;
        if (solved || tries >= a.reg_max_tries) break;
        lam *= 10.0;
      }
    }
    mask2(Qi, w, m, m);
    const bool fail_row = bad || !solved;

    // gains: K = -Quu_reg^-1 Qux, k = -Quu_reg^-1 Qu
    double K[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) K[r] = 0.0;
    prod2<false>(K, Qi, Qux, m, w);
#pragma unroll
    for (int r = 0; r < MR; ++r) K[r] = -K[r];
    mask2(K, w, m, n);
    const double kv = (c < m) ? -dot_col(Qi, qu, w) : 0.0;

    // value update
    double Vn[HR];
#pragma unroll
    for (int r = 0; r < HR; ++r) Vn[r] = Qxx[r];
    double vxn = qx, v0n = v0;
    if constexpr (MODE == 0) {
      vxn += dot_col(K, qu, w);            // + K^T Qu
      vxn += dot_col(Qux, kv, w);          // + Qux^T k
      const double qk = (c < m) ? dot_col(QuuT, kv, w) : 0.0;  // (Quu k)[c]
      vxn += dot_col(K, qk, w);            // + K^T Quu k
      double QK[MR];
#pragma unroll
      for (int r = 0; r < MR; ++r) QK[r] = Qux[r];
      prod2<false>(QK, Quu, K, m, w);      // Qux + Quu K
      mask2(QK, w, m, n);
      prod2<true>(Vn, K, QK, m, w);        // + K^T (Qux + Quu K)
      prod2<true>(Vn, Qux, K, m, w);       // + Qux^T K
    } else {
      prod2<true>(Vn, Qux, K, m, w);       // Qxx - Qux^T Quu^-1 Qux
      vxn += dot_col(Qux, kv, w);          // Qx - Qux^T Quu^-1 Qu
      v0n = l0 + v0 + 0.5 * vec_sum((c < m) ? qu * kv : 0.0);
    }
    vxn = (c < n) ? vxn : 0.0;
    mask2(Vn, w, n, n);
    symmetrize(Vn, w);
    // value_expansions (horizon_selection.py:209-210) raises on any non-finite V.  The
    // brute-force curve raises only through the next step's chol_solve: a non-finite
    // Vxx / Vx fails there, a non-finite V_0 never does, and at t = 0 nothing follows,
    // so only chol_solve(Quu_reg, Qux) itself can raise (Qux).
    bool vbad = !finite_val(vxn) || (!JC && !finite_val(v0n));
#pragma unroll
    for (int r = 0; r < HR; ++r) vbad = vbad || !finite_val(Vn[r]);
    if (JC && i == 0) {
      vbad = false;
#pragma unroll
      for (int r = 0; r < MR; ++r) vbad = vbad || !finite_val(Qux[r]);
    }
    const bool vfail = any_lane(vbad);

    if (fail_row || vfail) {
      st |= ST_FAIL;
      if (bad || vfail) st |= ST_NONFINITE;
      alive = false;
    } else {
#pragma unroll
      for (int r = 0; r < HR; ++r) Vxx[r] = Vn[r];
      vx = vxn;
      v0 = v0n;
      if constexpr (!JC) {
        store_cols(a.K + (prob * NA + i) * (long long)m * n, m, n, w, K);
        if (c < m && w.h == 0) a.k[(prob * NA + i) * m + c] = kv;
        if (a.Vxx) store_cols(a.Vxx + (prob * (NA + 1) + i) * nn, n, n, w, Vn);
        if (a.Vx && c < n && w.h == 0) a.Vx[prob * (NA + 1) * n + (long long)i * n + c] = vxn;
        if (a.V0 && lane == 0) a.V0[prob * (NA + 1) + i] = v0n;
      }
    }
  }
  if constexpr (JC) {  // V_0 of this horizon's sweep (the reference raises on failure: NaN)
    if (lane == 0) {
      const long long o = prob * a.jc_tmax + (L - 1);
      a.jc_J[o] = alive ? v0 : __builtin_nan("");
      a.jc_status[o] = (int)st;
    }
  } else {
    if (lane == 0) a.status[prob] = (int)st;
  }
}

template <int HR>
hipError_t launch_riccati_wide(const RiccatiArgs<double>& a, hipStream_t stream) {
  const long long blocks = (a.batch + kWavesPerBlockW - 1) / kWavesPerBlockW;
  const dim3 grid((unsigned)blocks), block(64 * kWavesPerBlockW);
  if (a.mode == 0) hipLaunchKernelGGL((riccati_wide_kernel<HR, 0>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((riccati_wide_kernel<HR, 1>), grid, block, 0, stream, a);
  return hipGetLastError();
}

template <int HR>
hipError_t launch_riccati_wide_jcurve(const RiccatiArgs<double>& a, hipStream_t stream) {
  const long long waves = a.batch * (long long)a.jc_tmax;
  const long long blocks = (waves + kWavesPerBlockW - 1) / kWavesPerBlockW;
  hipLaunchKernelGGL((riccati_wide_kernel<HR, 1, true>), dim3((unsigned)blocks),
                     dim3(64 * kWavesPerBlockW), 0, stream, a);
  return hipGetLastError();
}

hipError_t dispatch_riccati_wide_jcurve(const RiccatiArgs<double>& a, hipStream_t stream) {
  if (a.n <= 16) return launch_riccati_wide_jcurve<8>(a, stream);
  if (a.n <= 24) return launch_riccati_wide_jcurve<12>(a, stream);
  return launch_riccati_wide_jcurve<16>(a, stream);
}

hipError_t dispatch_riccati_wide(const RiccatiArgs<double>& a, hipStream_t stream) {
  if (a.n <= 16) return launch_riccati_wide<8>(a, stream);
  if (a.n <= 24) return launch_riccati_wide<12>(a, stream);
  return launch_riccati_wide<16>(a, stream);
}

}  // namespace wide
}  // namespace hop

extern "C" {

int hop_riccati_wide_f64(const double* A, const double* Bm, const double* X, const double* U,
                         const double* xg, int64_t xg_bs, const double* u_ref, int64_t ur_bs,
                         const double* Q, int64_t q_bs, const double* R, int64_t r_bs,
                         const double* Qf, int64_t qf_bs, const double* qxx_extra,
                         const double* qx_extra, const double* c_extra, const int32_t* horizon,
                         const double* lm, double w_stage, uint32_t wrap_mask, int32_t mode,
                         int32_t reg_max_tries, int64_t batch, int32_t n_alloc, int32_t n,
                         int32_t m, double* K, double* k, double* Vxx, double* Vx, double* V0,
                         int32_t* status, void* stream) {
  using hop::set_error;
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n < 1 || n > HOP_WIDE_MAX_DIM - 1) return set_error(HOP_E_SIZE, "n must be in [1, 31]");
  if (m < 1 || m > HOP_MAX_DIM) return set_error(HOP_E_SIZE, "m must be in [1, 16]");
  if (batch == 0) return HOP_OK;
  if (n_alloc < 1) return set_error(HOP_E_ARG, "n_alloc < 1");
  if (mode != 0 && mode != 1) return set_error(HOP_E_ARG, "mode must be 0 or 1");
  if (reg_max_tries < 1) return set_error(HOP_E_ARG, "reg_max_tries < 1");
  if ((wrap_mask >> n) != 0u) return set_error(HOP_E_ARG, "wrap_mask names a state >= n");
  if (xg_bs < 0 || ur_bs < 0 || q_bs < 0 || r_bs < 0 || qf_bs < 0)
    return set_error(HOP_E_ARG, "negative stride");
  if (!A || !Bm || !X || !U || !xg || !u_ref || !Q || !R || !Qf || !horizon || !lm || !K || !k ||
      !status)
    return set_error(HOP_E_ARG, "null pointer");
  if ((batch + hop::wide::kWavesPerBlockW - 1) / hop::wide::kWavesPerBlockW > 0x7fffffffLL)
    return set_error(HOP_E_SIZE, "batch too large for one launch");
  hop::RiccatiArgs<double> a;
  a.A = A; a.Bm = Bm; a.X = X; a.U = U; a.xg = xg; a.u_ref = u_ref; a.Q = Q; a.R = R; a.Qf = Qf;
  a.qxx_extra = qxx_extra; a.qx_extra = qx_extra; a.c_extra = c_extra;
  a.horizon = horizon; a.lm = lm;
  a.xg_bstride = xg_bs; a.uref_bstride = ur_bs; a.q_bstride = q_bs; a.r_bstride = r_bs;
  a.qf_bstride = qf_bs;
  a.batch = batch; a.nalloc = n_alloc; a.n = n; a.m = m; a.mode = mode;
  a.reg_max_tries = reg_max_tries; a.max_tries = 8; a.wrap_mask = wrap_mask; a.w_stage = w_stage;
  a.K = K; a.k = k; a.Vxx = Vxx; a.Vx = Vx; a.V0 = V0; a.status = status;
  return hop::set_hip_status(hop::wide::dispatch_riccati_wide(a, (hipStream_t)stream));
}

int hop_bruteforce_jcurve_wide_f64(const double* A, const double* Bm, const double* X,
                                   const double* U, const double* xg, int64_t xg_bs,
                                   const double* u_ref, int64_t ur_bs, const double* Q,
                                   int64_t q_bs, const double* R, int64_t r_bs, const double* Qf,
                                   int64_t qf_bs, const double* qxx_extra, const double* qx_extra,
                                   const double* c_extra, double lm_lambda, double w_stage,
                                   uint32_t wrap_mask, int64_t batch, int32_t n_alloc, int32_t n,
                                   int32_t m, int32_t t_max, double* J, int32_t* status,
                                   void* stream) {
  using hop::set_error;
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n < 1 || n > HOP_WIDE_MAX_DIM - 1) return set_error(HOP_E_SIZE, "n must be in [1, 31]");
  if (m < 1 || m > HOP_MAX_DIM) return set_error(HOP_E_SIZE, "m must be in [1, 16]");
  if (t_max < 1) return set_error(HOP_E_ARG, "t_max < 1");
  // the reference slices A_list[:T] for T <= T_max (an IndexError past N)
  if (t_max > n_alloc) return set_error(HOP_E_ARG, "t_max > n_alloc (reference IndexError)");
  if ((wrap_mask >> n) != 0u) return set_error(HOP_E_ARG, "wrap_mask names a state >= n");
  if (xg_bs < 0 || ur_bs < 0 || q_bs < 0 || r_bs < 0 || qf_bs < 0)
    return set_error(HOP_E_ARG, "negative stride");
  if (batch > 0 && (!A || !Bm || !X || !U || !xg || !u_ref || !Q || !R || !Qf || !J || !status))
    return set_error(HOP_E_ARG, "null pointer");
  // one wave64 per (problem, horizon), kWavesPerBlockW per workgroup: the dispatch limit
  // is in work-items, so the workgroups times their 64 kWavesPerBlockW lanes fit 32 bits
  constexpr long long kMaxWaves =
      0xFFFFFFFFll / (64 * hop::wide::kWavesPerBlockW) * hop::wide::kWavesPerBlockW;
  if (batch > kMaxWaves / t_max)
    return set_error(HOP_E_SIZE, "batch * t_max too large for one launch");
  if (batch == 0) return HOP_OK;
  hop::RiccatiArgs<double> a;
  a.A = A; a.Bm = Bm; a.X = X; a.U = U; a.xg = xg; a.u_ref = u_ref; a.Q = Q; a.R = R; a.Qf = Qf;
  a.qxx_extra = qxx_extra; a.qx_extra = qx_extra; a.c_extra = c_extra;
  a.horizon = nullptr; a.lm = nullptr;
  a.xg_bstride = xg_bs; a.uref_bstride = ur_bs; a.q_bstride = q_bs; a.r_bstride = r_bs;
  a.qf_bstride = qf_bs;
  a.batch = batch; a.nalloc = n_alloc; a.n = n; a.m = m; a.mode = 1;
  a.reg_max_tries = 1; a.max_tries = 8; a.wrap_mask = wrap_mask; a.w_stage = w_stage;
  a.K = nullptr; a.k = nullptr; a.Vxx = nullptr; a.Vx = nullptr; a.V0 = nullptr;
  a.status = nullptr;
  a.jc_J = J; a.jc_status = status; a.jc_tmax = t_max; a.lm_value = lm_lambda;
  return hop::set_hip_status(hop::wide::dispatch_riccati_wide_jcurve(a, (hipStream_t)stream));
}

}  // extern "C"
