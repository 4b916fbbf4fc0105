/*
 * hop_onepass.h -- the device primitives of the one-pass window method (baseline2,
 * method="onepass") of libhop_amd.so for the five built-in systems of hop.h: the
 * nominal cost curve, the negative-time prefix, the window pick and the rollout of the
 * shifted policy.  The backward sweep between them is hop_riccati_f64 (mode 1) on the
 * extended trajectory.  hop.h, hop_wide.h, hop_wide_jcurve.h and hop_chain.h keep their
 * entries; nothing here changes them, and the ABI version of hop.h covers this header too.
 *
 * Layout conventions, the memory contract (every output below is written whole; the byte
 * workspace is 8-byte aligned), error codes, streams and hop_last_error are those of hop.h; the
 * cost arguments (xg .. wrap_mask) are hop_cost_true_f64's, in its order.  fp64 only.
 * Every entry validates its arguments on the host before any launch:
 *   HOP_E_ARG  (-1)  unknown system, null pointers, negative sizes or strides, windows or
 *                    horizons out of range, n_alpha outside [1, 8], a workspace that is
 *                    too small
 *   HOP_E_SIZE (-2)  a state size that is none of the five systems' (2, 4, 12), S above
 *                    HOP_ONEPASS_MAX_WINDOW, a batch too large for one launch
 *   0, nothing launched, for batch = 0.
 */
#ifndef HOP_ONEPASS_H
#define HOP_ONEPASS_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_ONEPASS_MAX_WINDOW 64 /* S_left, S_right, the prefix length */

/*
 * hop_onepass_nominal_curve_f64
 * Replaces nominal_cost_curve (the reference's solver.py:108-149) and the argmin that
 *   follows it (solver.py:537) for a batch: X [batch][N+1][n], U [batch][N][m] ->
 *   J [batch][T_max], T_bar [batch].  J[b][k-1] = running_k + 0.5 e_k.Qf e_k for
 *   T_min <= k <= T_max and +inf elsewhere; the whole row is +inf when X[:T_max+1] or
 *   U[:T_max] holds a non-finite value.  Per step running += (0.5 e.Qe + 0.5 du.R du) + w,
 *   then + c_extra (the obstacle table).  T_bar[b] = the first argmin over [T_min, T_max]
 *   (T_min for an all-inf row).  1 <= T_min <= T_max <= N.
 */
int hop_onepass_nominal_curve_f64(int32_t system, const double* X, const double* U,
                                  const double* xg, int64_t xg_batch_stride, const double* u_ref,
                                  int64_t u_ref_batch_stride, const double* Q,
                                  int64_t q_batch_stride, const double* R, int64_t r_batch_stride,
                                  const double* Qf, int64_t qf_batch_stride, const double* w,
                                  int64_t w_batch_stride, const double* obstacles, int32_t n_obs,
                                  uint32_t wrap_mask, int32_t T_min, int32_t T_max, int64_t batch,
                                  int32_t N, double* J, int32_t* T_bar, void* stream);

/*
 * hop_onepass_extend_backward_f64
 * Replaces extend_nominal_backward with preimage_method="fixedpoint" (the reference's
 *   linearization.py:41-71, 109-170) for a batch: X [batch][N+1][n], U [batch][N][m],
 *   u_fill [batch][m] -> X_ext [batch][S+N+1][n], U_ext [batch][S+N][m], 1 <= S <=
 *   HOP_ONEPASS_MAX_WINDOW.  The tail is a copy of X, U; the prefix controls are u_fill.
 *   Prefix step s = 1 .. S starts at x = x_curr and runs max_iter iterations
 *   x -= damping (F(x, u_fill) - x_curr): a non-finite F breaks and keeps x,
 *   ||F - x_curr||_2 < tol returns x; a non-finite result falls back to x_curr.
 */
int hop_onepass_extend_backward_f64(int32_t system, double dt, const double* X, const double* U,
                                    const double* u_fill, int64_t batch, int32_t N, int32_t S,
                                    int32_t max_iter, double tol, double damping, double* X_ext,
                                    double* U_ext, void* stream);

/*
 * hop_onepass_pick_f64
 * Replaces onepass_pick_T_singlepass (the reference's horizon_selection.py:215-282) for a
 *   batch with per-problem T_bar [batch]: Vxx [batch][n_ext][n][n], Vx [batch][n_ext][n],
 *   V0 [batch][n_ext] (hop_riccati_f64 mode 1 on the extended trajectory, n_ext = its
 *   n_alloc + 1), X_ext [batch][n_ext][n], x0 [batch][n] -> T_star [batch],
 *   Jw [batch][T_max] (NaN where not evaluated).  Window [max(T_min, T_bar - S_left),
 *   min(T_max, T_bar + S_right)]; candidate T reads index i = T_bar - T + S_right and is
 *   skipped unless 0 <= i < n_ext; dx0 = wrap(x0 - X_ext[i]); candidates with
 *   ||dx0|| > locality_mult * median are gated out (NumPy's median of the norms that are
 *   finite and > 1e-12; no gate without one); J_T = 0.5 dx0.Vxx_i dx0 + Vx_i.dx0 + V0_i.
 *   The scan is centre-out, the smaller T first at equal distance, strict <.  A non-finite
 *   best gives clip(T_bar, L, R); L > R gives clip(T_bar, T_min, T_max) and an all-NaN row.
 *   S_right is the reference's argument: the shrink loop passes one below the arrays'
 *   offset, and i moves with it.  0 <= S_left, S_right <= HOP_ONEPASS_MAX_WINDOW,
 *   1 <= T_min <= T_max; n is 2, 4 or 12.
 */
int hop_onepass_pick_f64(const double* Vxx, const double* Vx, const double* V0,
                         const double* X_ext, const double* x0, const int32_t* T_bar,
                         int64_t batch, int32_t n, int32_t n_ext, int32_t T_min, int32_t T_max,
                         int32_t S_left, int32_t S_right, uint32_t wrap_mask,
                         double locality_mult, int32_t* T_star, double* Jw, void* stream);

/* bytes of workspace hop_onepass_rollout_f64 needs (0 for invalid arguments) */
size_t hop_onepass_rollout_workspace_bytes(int32_t system, int64_t batch, int32_t N,
                                           int32_t n_alpha);

/*
 * hop_onepass_rollout_f64
 * Replaces onepass_rollout (the reference's solver.py:365-442) for a batch:
 *   X_ext [batch][S+N+1][n], U_ext [batch][S+N][m], K [batch][S+N][m][n],
 *   k [batch][S+N][m] (hop_riccati_f64 mode 1), T_bar, T_star [batch], S = the arrays'
 *   offset.  Every (problem, alpha) pair is rolled out side by side from X_ext[S] over N
 *   steps: for t < T* the control is U_ext[idx] + K[idx] wrap(x_t - X_ext[idx]) +
 *   alpha k[idx] with idx = T_bar - T* + t + S, for t >= T* the unshifted U_ext[S + t].
 *   A non-finite state drops that alpha; J is cost_timeopt_true at T*.  The smallest J
 *   wins (strict < in alpha order: ties keep the earlier alpha).  accepted [batch] = that
 *   index; -1 when no alpha gave J < +inf; -2 for a problem that is inactive
 *   (active[b] == 0, nullable = all active) or whose indices leave the arrays
 *   (T* outside [0, N], T_bar outside [0, N], T* > T_bar + S).  For -1 and -2, J = +inf
 *   and X_new, U_new are the nominal tail X_ext[S:], U_ext[S:].  alphas: n_alpha host
 *   doubles, 1 <= n_alpha <= 8.
 */
int hop_onepass_rollout_f64(int32_t system, double dt, const double* X_ext, const double* U_ext,
                            const double* xg, int64_t xg_batch_stride, const double* u_ref,
                            int64_t u_ref_batch_stride, const double* Q, int64_t q_batch_stride,
                            const double* R, int64_t r_batch_stride, const double* Qf,
                            int64_t qf_batch_stride, const double* w, int64_t w_batch_stride,
                            const double* obstacles, int32_t n_obs, uint32_t wrap_mask,
                            const int32_t* T_bar, const int32_t* T_star, const int32_t* active,
                            const double* K, const double* k, const double* alphas,
                            int32_t n_alpha, int64_t batch, int32_t N, int32_t S, void* workspace,
                            size_t workspace_bytes, double* X_new, double* U_new, double* J,
                            int32_t* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_ONEPASS_H */
