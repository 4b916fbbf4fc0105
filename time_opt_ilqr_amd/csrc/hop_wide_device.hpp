// Device primitives of the wide path (17 <= s <= 32, fp64): one problem per wave64.
//
// Data layout: lane (c, h), c = lane & 31, h = lane >> 5, holds rows h HR .. h HR + HR - 1
// of column c of every s x s matrix (HR = rows per half, s <= 2 HR), so a matrix costs
// HR registers per lane whatever s is.  Entries outside the s x s block are exact
// zeros (every primitive re-establishes that), so no identity padding is needed.
//
// A product goes through two LDS images per wave: the left factor stored so that the
// HR values a lane needs for one contraction index j are contiguous (one address per
// half wave: the reads broadcast, two doubles per ds_read_b128), the right factor row
// by row (lane c reads its own column, conflict-free).  The contraction loop runs to
// the real s, not to the padded size.  No 16-lane DPP rows are involved; the narrow
// kernels' RowB / LaneB chains stay for s <= 16.
#pragma once
#include "hop_device.hpp"

namespace hop {
namespace wide {

constexpr int kLd = 34;             // image row stride in doubles (even: 16-byte rows)
constexpr int kImg = 32 * kLd;      // one 32 x 32 image
constexpr int kBtLd = 17;           // row stride of the B_k staging tile (32 x 16)
constexpr int kRinvLd = 16;         // row stride of the R^-1 tile (16 x 16)
// per-wave LDS, in doubles: left image, right image, pivot column, R^-1, B_k rows
constexpr int kLdsWave = 2 * kImg + 32 + 16 * kRinvLd + 32 * kBtLd;
constexpr int kWavesPerBlockW = 2;  // 128-thread workgroups: 2 * 24064 B of LDS

struct Ctx {
  double* L;     // left image
  double* Y;     // right image
  double* col;   // pivot column of the sweep
  double* rinv;  // R^-1
  double* bt;    // B_k rows
  int c, h, s;
};

template <int HR>
__device__ __forceinline__ bool live(const Ctx& w, int i) {
  return (w.h * HR + i < w.s) && (w.c < w.s);
}
// zero everything outside the s x s block (0 * NaN of a product's padding, the sweep's
// untouched padding lanes)
template <int HR>
__device__ __forceinline__ void mask(double (&x)[HR], const Ctx& w) {
#pragma unroll
  for (int i = 0; i < HR; ++i) x[i] = live<HR>(w, i) ? x[i] : 0.0;
}
// buf[row][c] = x
template <int HR>
__device__ __forceinline__ void put(double* buf, const double (&x)[HR], const Ctx& w) {
#pragma unroll
  for (int i = 0; i < HR; ++i) buf[(w.h * HR + i) * kLd + w.c] = x[i];
}
// buf[c][row] = x
template <int HR>
__device__ __forceinline__ void put_t(double* buf, const double (&x)[HR], const Ctx& w) {
  double2* p = reinterpret_cast<double2*>(buf + w.c * kLd + w.h * HR);
#pragma unroll
  for (int i = 0; i < HR / 2; ++i) p[i] = make_double2(x[2 * i], x[2 * i + 1]);
}
// x = buf[c][row]
template <int HR>
__device__ __forceinline__ void get_t(const double* buf, double (&x)[HR], const Ctx& w) {
  const double2* p = reinterpret_cast<const double2*>(buf + w.c * kLd + w.h * HR);
#pragma unroll
  for (int i = 0; i < HR / 2; ++i) {
    const double2 v = p[i];
    x[2 * i] = v.x;
    x[2 * i + 1] = v.y;
  }
}

// out[row] (+/-)= sum_{j < cnt} L[j][row] * Y[j][c]
template <bool NEG, int HR>
__device__ __forceinline__ void mul(double (&out)[HR], const double* L, const double* Y, int cnt,
                                    const Ctx& w) {
  const double* pl = L + w.h * HR;
  const double* py = Y + w.c;
#pragma unroll 2
  for (int j = 0; j < cnt; ++j) {
    const double y0 = py[j * kLd];
    const double yv = NEG ? -y0 : y0;
    const double2* p = reinterpret_cast<const double2*>(pl + j * kLd);
#pragma unroll
    for (int i = 0; i < HR / 2; ++i) {
      const double2 v = p[i];
      out[2 * i] = __builtin_fma(v.x, yv, out[2 * i]);
      out[2 * i + 1] = __builtin_fma(v.y, yv, out[2 * i + 1]);
    }
  }
}

// out (+/-)= X Y (XT = false) or X^T Y (XT = true); x, y, out in the register layout
template <bool XT, bool NEG, int HR>
__device__ __forceinline__ void prod(double (&out)[HR], const double (&x)[HR],
                                     const double (&y)[HR], const Ctx& w) {
  if constexpr (XT) put(w.L, x, w);  // L[j][r] = X[j][r]
  else put_t(w.L, x, w);             // L[j][r] = X[r][j]
  put(w.Y, y, w);
  wave_sync();
  mul<NEG>(out, w.L, w.Y, w.s, w);
  wave_sync();
  mask(out, w);
}

// One pivot p = PH HR + PI of the symmetric sweep operator (hop_device.hpp's
// sweep_pivot) on (M + eps I).  The register index PI is a compile-time constant, so
// row p is the lane's own register PI or its partner half's (one cross-half exchange)
// and only that register is overwritten: no select chains over the HR registers.
// Column p goes through LDS (lane p writes it, every lane reads its HR rows of it: one
// address per half wave, two doubles per read).
template <int PI, int HR>
__device__ __forceinline__ void sweep_pivot_w(double (&r)[HR], double eps, const Ctx& w, int ph,
                                              bool& ok) {
  const int p = ph * HR + PI;
  const double ro = __shfl_xor(r[PI], 32);
  const double apc = (w.h == ph) ? r[PI] : ro;  // a_pc
  if (w.c == p) {
    double2* pw = reinterpret_cast<double2*>(w.col + w.h * HR);
#pragma unroll
    for (int i = 0; i < HR / 2; ++i) pw[i] = make_double2(r[2 * i], r[2 * i + 1]);
  }
  wave_sync();
  const double d = w.col[p] + eps;
  ok = ok && (d > 0.0);
  const double rd = recip_nr(d);
  const bool piv = (w.c == p);
  const double sc = piv ? 0.0 : -apc * rd;
  const double rowp = piv ? -rd : apc * rd;
  const double f = piv ? rd : 1.0;
  const double2* pc = reinterpret_cast<const double2*>(w.col + w.h * HR);
#pragma unroll
  for (int i = 0; i < HR / 2; ++i) {
    const double2 a = pc[i];
    r[2 * i] = __builtin_fma(a.x, sc, r[2 * i]) * f;          // a_ic -= a_ip a_pc / d
    r[2 * i + 1] = __builtin_fma(a.y, sc, r[2 * i + 1]) * f;  // (column p: a_ip / d)
  }
  r[PI] = (w.h == ph) ? rowp : r[PI];
  wave_sync();
}

// r <- -(M + eps I)^-1, pivots 0 .. s-1 (the padding needs none: it is zero and stays
// zero).  ok: every pivot d > 0 (potrf's rejection test).
template <int HR>
__device__ __forceinline__ void sweep_neg_inverse(double (&r)[HR], double eps, const Ctx& w,
                                                  bool& ok) {
#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {
    static_for<HR>([&](auto P) {
      constexpr int pi = P;
      if (ph * HR + pi < w.s) sweep_pivot_w<pi>(r, eps, w, ph, ok);  // wave-uniform
    });
  }
}

// chol_inv's LU slot (utils.py:88-93) for one problem per wave: gesv on
// A = sym(M) + eps I with the identity as right-hand side, in LDS: the caller has put
// A into L and the identity into Y, the inverse is left in Y.  Half 0 owns the columns
// of A, half 1 the columns of X; a lane touches only its own column, and column p of A is left as it
// is during step p (nothing reads it afterwards), so a step needs one synchronisation
// after the row exchange and one at its end.  Partial pivoting as idamax (the first
// row of largest |a_ip|).  Returns false on an exactly zero pivot (LinAlgError).
__device__ __noinline__ bool lu_wave(double* L, double* Y, int s, double eps, int c, int h) {
  double* M = h ? Y : L;
  const bool mine = c < s;
  bool ok = true;
  for (int p = 0; p < s; ++p) {
    int piv = p;
    double big = __builtin_fabs(L[p * kLd + p]);
    for (int i = p + 1; i < s; ++i) {
      const double v = __builtin_fabs(L[i * kLd + p]);
      if (v > big) {
        big = v;
        piv = i;
      }
    }
    wave_sync();  // every lane has scanned column p
    if (piv != p && mine) {
      const double t = M[p * kLd + c];
      M[p * kLd + c] = M[piv * kLd + c];
      M[piv * kLd + c] = t;
    }
    wave_sync();
    const double d = L[p * kLd + p];
    if (!(d != 0.0)) {
      ok = false;
      continue;
    }
    if (mine && !(h == 0 && c == p)) {
      const double mp = M[p * kLd + c];
      for (int i = p + 1; i < s; ++i) {
        const double l = L[i * kLd + p] / d;
        M[i * kLd + c] -= l * mp;
      }
    }
    wave_sync();
  }
  if (ok && h == 1 && mine) {
    for (int i = s - 1; i >= 0; --i) {
      double v = Y[i * kLd + c];
      for (int j = i + 1; j < s; ++j) v -= L[i * kLd + j] * Y[j * kLd + c];
      Y[i * kLd + c] = v / L[i * kLd + i];
    }
  }
  wave_sync();
  return ok;
}

// In place: r <- (sym(r) + eps I)^-1 with hop_device.hpp's sym_spd_inverse semantics
// (utils.py:69-93): eps = 1e-9, x10 per failed factorisation, up to max_tries, then the
// LU slot; a non-finite input gives NaN and ST_NONFINITE without a ladder.  The input
// is parked in the left image for retries and the LU slot.  A wave is one problem, so
// every decision is wave-uniform.
template <int HR>
__device__ __forceinline__ void sym_spd_inverse(double (&r)[HR], const Ctx& w, int max_tries,
                                                unsigned& st) {
  put(w.L, r, w);
  wave_sync();
  {
    double t[HR];
    get_t(w.L, t, w);
    // for HR < 16 the lanes c >= 2 HR read rows this put has not written (what the
    // kernel before left in LDS): only values from inside the block enter the registers
#pragma unroll
    for (int i = 0; i < HR; ++i) r[i] = live<HR>(w, i) ? 0.5 * (r[i] + t[i]) : 0.0;
  }
  double eps = 1e-9;
  int tries = 0;
  bool nf = false, lu = false;
#pragma unroll 1
  while (true) {
    bool ok = true;
    sweep_neg_inverse(r, eps, w, ok);
    if (ok) break;
    if (tries == 0) {  // chol_inv's _assert_finite (utils.py:75)
      double z = 0.0;
#pragma unroll
      for (int i = 0; i < HR; ++i) z = z + w.L[(w.h * HR + i) * kLd + w.c] * 0.0;
      nf = __any(!(z == z)) != 0;
      if (nf) {
        st |= ST_NONFINITE;
        break;
      }
    }
    if (tries >= max_tries) {
      st |= ST_LU;
      lu = true;
      break;
    }
    eps *= 10.0;
    ++tries;
    st |= ST_JITTER;
    double t[HR];
    get_t(w.L, t, w);
#pragma unroll
    for (int i = 0; i < HR; ++i)
      r[i] = live<HR>(w, i) ? 0.5 * (w.L[(w.h * HR + i) * kLd + w.c] + t[i]) : 0.0;
  }
  bool okl = true;
  if (lu) {
    double a[HR];
    get_t(w.L, a, w);
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const bool dg = live<HR>(w, i) && (w.h * HR + i == w.c);
      a[i] = live<HR>(w, i)
                 ? 0.5 * (w.L[(w.h * HR + i) * kLd + w.c] + a[i]) + (dg ? eps : 0.0) : 0.0;
    }
    wave_sync();
    put(w.L, a, w);
#pragma unroll
    for (int i = 0; i < HR; ++i)
      a[i] = (live<HR>(w, i) && (w.h * HR + i == w.c)) ? 1.0 : 0.0;
    put(w.Y, a, w);
    wave_sync();
    okl = lu_wave(w.L, w.Y, w.s, eps, w.c, w.h);
#pragma unroll
    for (int i = 0; i < HR; ++i) r[i] = -w.Y[(w.h * HR + i) * kLd + w.c];
  }
  const bool bad = nf || !okl;
#pragma unroll
  for (int i = 0; i < HR; ++i) r[i] = bad ? __builtin_nan("") : -r[i];
  mask(r, w);
}

}  // namespace wide
}  // namespace hop
