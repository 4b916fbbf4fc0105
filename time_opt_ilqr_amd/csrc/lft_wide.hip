// Wide LFT horizon sweep (17 <= s <= 32, fp64; accepts 1 <= s <= 32): the association
// of lft_sweep.hip, one problem per wave64 (hop_wide_device.hpp).  Per step k
//   stage   E_k = (Q_k+eps)^-1, F_k = E_k A_k^T, G_k = A_k F_k + B_k R^-1 B_k^T
//   compose W = (E_k + Gbar)^-1, Ebar -= Fbar W Fbar^T, Fbar = Fbar W F_k,
//           Gbar = G_k - F_k^T W F_k
//   query   J_{k+1} = 1/2 z0^T (Ebar - Fbar (QT_k^-1 + Gbar)^-1 Fbar^T)^-1 z0
// Reference: horizon_selection.py:36-86 (propagator_all_Jt_aug), the argmin of
// solver.py:522 fused as an option.  Fbar is carried transposed (H = Fbar^T).
// No workgroup barrier anywhere: the two waves of a workgroup never meet, so a wave
// without a problem simply returns.
#include "hop_wide_device.hpp"
#include "hop_kernels.hpp"
#include "../../include/hop_wide.h"

namespace hop {
namespace wide {

template <int HR>
__device__ __forceinline__ void load_col(const double* M, const Ctx& w, double (&x)[HR]) {
#pragma unroll
  for (int i = 0; i < HR; ++i) {
    const bool in = live<HR>(w, i);
    const double v = M[in ? (w.h * HR + i) * w.s + w.c : 0];
    x[i] = in ? v : 0.0;
  }
}
// x = M^T in the register layout: x[row] = M[c][row]
template <int HR>
__device__ __forceinline__ void load_row(const double* M, const Ctx& w, double (&x)[HR]) {
#pragma unroll
  for (int i = 0; i < HR; ++i) {
    const bool in = live<HR>(w, i);
    const double v = M[in ? w.c * w.s + w.h * HR + i : 0];
    x[i] = in ? v : 0.0;
  }
}
template <int HR>
__device__ __forceinline__ void store_col(double* M, const Ctx& w, const double (&x)[HR]) {
#pragma unroll
  for (int i = 0; i < HR; ++i)
    if (live<HR>(w, i)) M[(w.h * HR + i) * w.s + w.c] = x[i];
}
template <int HR>
__device__ __forceinline__ void store_col_t(double* M, const Ctx& w, const double (&x)[HR]) {
#pragma unroll
  for (int i = 0; i < HR; ++i)
    if (live<HR>(w, i)) M[w.c * w.s + w.h * HR + i] = x[i];
}

__device__ __forceinline__ void load_rinv(const double* R, int m, int lane, const Ctx& w) {
  for (int e = lane; e < m * m; e += 64) w.rinv[(e / m) * kRinvLd + e % m] = R[e];
  wave_sync();
}

// G += (B R^-1) B^T: the left image takes (B R^-1)^T, the right image B^T, contraction m
template <int HR>
__device__ __forceinline__ void add_brb(double (&G)[HR], const double* Bk, int m, const Ctx& w) {
  const bool in = w.c < w.s;
  for (int l = w.h; l < m; l += 2) {
    const double v = in ? Bk[w.c * m + l] : 0.0;
    w.bt[w.c * kBtLd + l] = v;
    w.Y[l * kLd + w.c] = v;
  }
  wave_sync();
  for (int j = w.h; j < m; j += 2) {
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc = __builtin_fma(w.bt[w.c * kBtLd + l], w.rinv[l * kRinvLd + j], acc);
    w.L[j * kLd + w.c] = acc;
  }
  wave_sync();
  mul<false>(G, w.L, w.Y, m, w);
  wave_sync();
  mask(G, w);
}

template <int HR>
__global__ __launch_bounds__(64 * kWavesPerBlockW) void lft_wide_kernel(LftArgs<double> a) {
  __shared__ __attribute__((aligned(16))) double smem[kWavesPerBlockW * kLdsWave];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long prob = (long long)blockIdx.x * kWavesPerBlockW + wv;
  if (prob >= a.batch) return;  // wave-uniform
  Ctx w;
  w.L = smem + wv * kLdsWave;
  w.Y = w.L + kImg;
  w.col = w.Y + kImg;
  w.rinv = w.col + 32;
  w.bt = w.rinv + 16 * kRinvLd;
  w.c = lane & 31;
  w.h = lane >> 5;
  w.s = a.s;

  const int s = a.s, m = a.m, N = a.n, mt = a.max_tries;
  const long long ss = (long long)s * s, sm = (long long)s * m;
  const double* Ap = a.A + prob * a.nalloc * ss;
  const double* Bp = a.B + prob * a.nalloc * sm;
  const double* Qp = a.Q + prob * a.nalloc * ss;
  const double* QTp = a.QT + prob * a.nalloc * ss;
  const double* Rp = a.R + prob * a.r_bstride;
  const double* zp = a.z0 + prob * a.z_bstride;

  const double zc = (w.c < s) ? zp[w.c < s ? w.c : 0] : 0.0;

  unsigned st = 0;
  const bool r_fixed = (a.r_kstride == 0);
  if (r_fixed) load_rinv(Rp, m, lane, w);

  double Eb[HR], H[HR], Gb[HR];
  double best = 0.0;
  int tbest = 0;
  const bool fuse_argmin = a.t_max > 0;

#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    const double* Ak = Ap + k * ss;
    if (!r_fixed) load_rinv(Rp + k * a.r_kstride, m, lane, w);

    // ---- stage: E, F = E A^T; W = (E + Gbar)^-1 while the old Gbar is still there;
    //      then G = A F + B R^-1 B^T straight into Gbar's registers
    double F[HR], W[HR];
    double* dbg = a.dbg_efg != nullptr ? a.dbg_efg + ((prob * N + k) * 3) * ss : nullptr;
    {
      double E[HR];
      load_col(Qp + k * ss, w, E);
      sym_spd_inverse(E, w, mt, st);
      if (dbg) store_col(dbg, w, E);
      double at[HR];
      load_row(Ak, w, at);
#pragma unroll
      for (int i = 0; i < HR; ++i) F[i] = 0.0;
      prod<false, false>(F, E, at, w);
      if (dbg) store_col(dbg + ss, w, F);
      if (k == 0) {
#pragma unroll
        for (int i = 0; i < HR; ++i) Eb[i] = E[i];
      } else {
#pragma unroll
        for (int i = 0; i < HR; ++i) W[i] = E[i] + Gb[i];
        sym_spd_inverse(W, w, mt, st);     // W = (E_k + Gbar)^-1
      }
#pragma unroll
      for (int i = 0; i < HR; ++i) Gb[i] = 0.0;
      prod<true, false>(Gb, at, F, w);     // A F
    }
    add_brb(Gb, Bp + k * sm, m, w);
    if (dbg) store_col(dbg + 2 * ss, w, Gb);

    // ---- compose the prefix (Ebar, H = Fbar^T, Gbar)
    if (k == 0) {
      put_t(w.L, F, w);
      wave_sync();
#pragma unroll
      for (int i = 0; i < HR; ++i) H[i] = w.L[(w.h * HR + i) * kLd + w.c];
      wave_sync();
    } else {
      double Z[HR];
#pragma unroll
      for (int i = 0; i < HR; ++i) Z[i] = 0.0;
      prod<false, false>(Z, W, H, w);      // Z = W Fbar^T
      prod<true, true>(Eb, H, Z, w);       // Ebar -= Fbar W Fbar^T
#pragma unroll
      for (int i = 0; i < HR; ++i) H[i] = 0.0;
      prod<true, false>(H, F, Z, w);       // H' = F^T W Fbar^T
#pragma unroll
      for (int i = 0; i < HR; ++i) Z[i] = 0.0;
      prod<false, false>(Z, W, F, w);      // W F
      prod<true, true>(Gb, F, Z, w);       // Gbar = G - F^T W F
    }
    if (a.dbg_pre != nullptr) {
      double* o = a.dbg_pre + ((prob * N + k) * 3) * ss;
      store_col(o, w, Eb);
      store_col_t(o + ss, w, H);
      store_col(o + 2 * ss, w, Gb);
    }

    // ---- query horizon t = k + 1
    double Xt[HR], V[HR];
    load_col(QTp + k * ss, w, Xt);
    sym_spd_inverse(Xt, w, mt, st);        // QT_k^-1
#pragma unroll
    for (int i = 0; i < HR; ++i) Xt[i] += Gb[i];
    sym_spd_inverse(Xt, w, mt, st);        // Wt = (QT^-1 + Gbar)^-1
#pragma unroll
    for (int i = 0; i < HR; ++i) V[i] = 0.0;
    prod<false, false>(V, Xt, H, w);       // Wt Fbar^T
#pragma unroll
    for (int i = 0; i < HR; ++i) Xt[i] = Eb[i];
    prod<true, true>(Xt, H, V, w);         // X0 = Ebar - Fbar Wt Fbar^T
    sym_spd_inverse(Xt, w, mt, st);        // P0 = X0^-1
    double u = 0.0;
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int r = w.h * HR + i;
      u = __builtin_fma((r < s) ? zp[r < s ? r : 0] : 0.0, Xt[i], u);
    }
    double v = u * zc;
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    const double jk = 0.5 * v;
    if (!finite_val(jk)) st |= ST_NONFINITE;
    if (lane == 0) a.J[prob * N + k] = jk;
    if (fuse_argmin) {
      const int t = k + 1;
      if (t == a.t_min) {
        best = jk;
        tbest = t;
      } else if (t > a.t_min && t <= a.t_max) {
        const bool bnan = best != best, jnan = jk != jk;
        if (!bnan && (jnan || jk < best)) {
          best = jk;
          tbest = t;
        }
      }
    }
  }
  if (lane == 0) {
    a.status[prob] = (int)st;
    if (fuse_argmin && a.t_star != nullptr) {
      a.t_star[prob] = tbest;
      a.j_star[prob] = best;
    }
  }
}

template <int HR>
hipError_t launch_lft_wide(const LftArgs<double>& a, hipStream_t stream) {
  const long long blocks = (a.batch + kWavesPerBlockW - 1) / kWavesPerBlockW;
  hipLaunchKernelGGL((lft_wide_kernel<HR>), dim3((unsigned)blocks), dim3(64 * kWavesPerBlockW), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t dispatch_lft_wide(const LftArgs<double>& a, hipStream_t stream) {
  if (a.s <= 16) return launch_lft_wide<8>(a, stream);
  if (a.s <= 20) return launch_lft_wide<10>(a, stream);
  if (a.s <= 24) return launch_lft_wide<12>(a, stream);
  if (a.s <= 28) return launch_lft_wide<14>(a, stream);
  return launch_lft_wide<16>(a, stream);
}

}  // namespace wide
}  // namespace hop

extern "C" {

int hop_lft_sweep_wide_f64(const double* A, const double* B, const double* Q, const double* R_inv,
                           int64_t r_bs, int64_t r_ks, int32_t r_is_inverse, const double* QT,
                           const double* z0, int64_t z_bs, int64_t batch, int32_t n_alloc,
                           int32_t n_use, int32_t s, int32_t m, int32_t max_tries, int32_t t_min,
                           int32_t t_max, double* J, int32_t* status, int32_t* t_star,
                           double* j_star, double* dbg_efg, double* dbg_pre, void* stream) {
  using hop::set_error;
  if (batch < 0) return set_error(HOP_E_ARG, "batch < 0");
  if (n_use <= 0 || batch == 0) return HOP_OK;  // reference: empty J
  if (s < 1 || s > HOP_WIDE_MAX_DIM) return set_error(HOP_E_SIZE, "s must be in [1, 32]");
  if (m < 1 || m > HOP_MAX_DIM) return set_error(HOP_E_SIZE, "m must be in [1, 16]");
  if (!r_is_inverse)
    return set_error(HOP_E_ARG, "wide sweep: R must be R^-1 (r_is_inverse = 1)");
  if (n_use > n_alloc) return set_error(HOP_E_ARG, "n_use > n_alloc (reference IndexError)");
  if (!A || !B || !Q || !QT || !z0 || !R_inv || !J || !status)
    return set_error(HOP_E_ARG, "null input/output pointer");
  if (r_bs < 0 || r_ks < 0 || z_bs < 0) return set_error(HOP_E_ARG, "negative stride");
  if (max_tries < 0 || max_tries > 64) return set_error(HOP_E_ARG, "max_tries out of range");
  if (t_max > 0) {
    if (t_min < 1 || t_min > t_max || t_max > n_use)
      return set_error(HOP_E_ARG, "need 1 <= t_min <= t_max <= n_use for the fused argmin");
    if (!t_star || !j_star) return set_error(HOP_E_ARG, "t_star/j_star required when t_max > 0");
  }
  if ((batch + hop::wide::kWavesPerBlockW - 1) / hop::wide::kWavesPerBlockW > 0x7fffffffLL)
    return set_error(HOP_E_SIZE, "batch too large for one launch");
  hop::LftArgs<double> a{};
  a.A = A; a.B = B; a.Q = Q; a.R = R_inv; a.QT = QT; a.z0 = z0;
  a.r_bstride = r_bs; a.r_kstride = r_ks; a.z_bstride = z_bs;
  a.batch = batch; a.nalloc = n_alloc; a.n = n_use; a.s = s; a.m = m;
  a.max_tries = max_tries; a.r_is_inv = 1;
  a.t_min = t_min; a.t_max = t_max;
  a.J = J; a.status = status; a.t_star = t_star; a.j_star = j_star;
  a.dbg_efg = dbg_efg; a.dbg_pre = dbg_pre;
  return hop::set_hip_status(hop::wide::dispatch_lft_wide(a, (hipStream_t)stream));
}

}  // extern "C"
