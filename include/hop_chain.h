/*
 * hop_chain.h -- the mass-spring chain as a device system of libhop_amd.so: the
 * dynamics, rollout, finite-difference linearisation, true cost and forward line
 * search of a chain whose size is a RUN-TIME argument (the five systems of hop.h are
 * template constants).  With these a wide solve (up to 30 states) runs end to end on
 * the device.  hop.h, hop_wide.h and hop_wide_jcurve.h keep their entries; nothing here
 * changes them, and the ABI version of hop.h covers this header too.
 *
 * The system (tests/golden/make_golden_wide.py, chain_dynamics):
 *   x = [q (p positions), v (p velocities)], n = 2 p; unit masses in a chain fixed at
 *   both ends; spring force k d + ks sin(d) on the stretch d; damping c; input j pushes
 *   mass j * p / m (integer division); one explicit Euler step of length dt:
 *     d_i = q_i - q_{i-1} (q_{-1} = q_p = 0),  f_i = (k d_i) + (ks sin d_i),
 *     acc_i = (f_{i+1} - f_i) - c v_i (+ u_j),  q' = q + dt v,  v' = v + dt acc.
 *   Evaluated in that order without FMA contraction: sin is the only operation that can
 *   differ from NumPy, and the q' half of F is bit-identical to it.
 *
 * Layout conventions, the memory contract (element alignment, written extents, inputs
 * never written), error codes, streams and hop_last_error are those of hop.h.
 * Every entry validates its arguments on the host before any launch:
 *   HOP_E_SIZE (-2)  p outside [1, HOP_CHAIN_MAX_P] or m outside [1, p]
 *   HOP_E_ARG  (-1)  null pointers, n_use > n_alloc, n_alpha outside [1, 8], dt <= 0,
 *                    negative sizes or strides (n_alloc < 0 too, whatever n_use is, as in
 *                    hop_fleet.h), a workspace that is too small
 *   0, nothing launched, for batch = 0 (count = 0, n_use = 0).
 * Any batch size and any N are accepted.
 */
#ifndef HOP_CHAIN_H
#define HOP_CHAIN_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_CHAIN_MAX_P 15 /* masses: p + 1 springs fill one 16-lane row */

/* The chain's parameters: a host struct, read before the launch. */
typedef struct hop_chain_params {
  int32_t p;  /* masses, 1 <= p <= HOP_CHAIN_MAX_P; n = 2 p states */
  int32_t m;  /* inputs, 1 <= m <= p */
  double dt;  /* Euler step, > 0 */
  double k;   /* linear spring constant */
  double ks;  /* coefficient of the sine term */
  double c;   /* damping */
} hop_chain_params;

/*
 * hop_chain_dynamics_f64
 * Replaces one call F(x, u) of chain_dynamics (make_golden_wide.py:54-74) per row, for
 *   `count` rows: X + r * x_stride [n], U + r * u_stride [m] -> Xn + r * xn_stride [n]
 *   (strides in elements, >= n / m / n).  The argument list is hop_dynamics_f64's with
 *   the parameters in place of (system, dt).
 */
int hop_chain_dynamics_f64(const hop_chain_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream);

/*
 * hop_chain_rollout_f64
 * Replaces rollout(F, x0, U, max_state_norm) (the reference's solver.py:42-62) for a
 *   batch: x0 [batch or 1][n] (x0_batch_stride 0 = shared), U [batch][N][m] ->
 *   X [batch][N+1][n].  The first state that is not finite or has ||x|| >
 *   max_state_norm and every state after it are NaN.  hop_rollout_f64's arguments.
 */
int hop_chain_rollout_f64(const hop_chain_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream);

/*
 * hop_chain_linearize_f64
 * Replaces linearize_central_diff_traj / linearize_forward_diff_traj and
 *   compute_affine_residuals (the reference's linearization.py:177-270) for a batch:
 *   X [batch][n_alloc+1][n], U [batch][n_alloc][m] -> A [batch][n_alloc][n][n],
 *   B [batch][n_alloc][n][m], a_res [batch][n_alloc][n] = F(x_k, u_k) - x_{k+1}
 *   (nullable), Fx [batch][n_alloc][n] = F(x_k, u_k) (nullable): the layout the
 *   augment, sweep and Riccati entries read.  Steps k < n_use are written, the others
 *   are left untouched.  h = max(eps, rel * max(1, |v|)) with Python's max.  Only the
 *   entries a column can reach cost a spring evaluation; every other entry is the
 *   quotient of two identical numbers (an exact zero, NaN where that output is not
 *   finite), as in the reference.  The forward form writes an all-NaN (A_k, B_k) when
 *   F(x_k, u_k) is not finite.  hop_linearize_f64's arguments.
 */
int hop_chain_linearize_f64(const hop_chain_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream);

/*
 * hop_chain_cost_true_f64
 * Replaces cost_timeopt_true (the reference's solver.py:65-102) for a batch at the
 *   per-problem horizons T_star [batch], with hop_cost_true_f64's conventions: +inf for
 *   T <= 0 or non-finite data on the rows read, NaN for T > N.  xg [batch or 1][n],
 *   u_ref [batch or 1][m] and w [batch or 1] take a batch stride (0 = shared); Q [n][n],
 *   R [m][m] and Qf [n][n] (the terminal weight, expanded) are shared by the batch.
 *   The chain has no angle and no planar position: there is no wrap mask and no
 *   obstacle table.
 */
int hop_chain_cost_true_f64(const hop_chain_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, int64_t batch, int32_t N, double* J,
                            void* stream);

/* bytes of workspace hop_chain_forward_linesearch_f64 needs (0 for invalid arguments) */
size_t hop_chain_forward_workspace_bytes(const hop_chain_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha);

/*
 * hop_chain_forward_linesearch_f64
 * Replaces forward_linesearch_fixedT (the reference's solver.py:233-286) for a batch,
 *   with hop_forward_linesearch_f64's result conventions: every (problem, alpha) pair is
 *   rolled out side by side over all N steps (controls U_k + K_k dx + alpha k_k for
 *   k < T*, U_k beyond), a non-finite state rejects that alpha, and the smallest index
 *   with J' < J_old strictly wins.  accepted [batch] = that index, -1 for none, -2 for
 *   an inactive problem (active[b] == 0, nullable = all active; T* outside [0, N]),
 *   whose X, U are copied through and whose J is J_old.  K [batch][N][m][n] and
 *   k [batch][N][m] as the Riccati entries' mode 0 writes them; alphas: n_alpha host
 *   doubles.  The cost arguments are hop_chain_cost_true_f64's.  The rollout arithmetic
 *   is hop_chain_rollout_f64's: with K = 0 and k = 0 the candidate is X bit for bit.
 */
int hop_chain_forward_linesearch_f64(const hop_chain_params* params, const double* X,
                                     const double* U, const double* xg, int64_t xg_batch_stride,
                                     const double* u_ref, int64_t u_ref_batch_stride,
                                     const double* Q, const double* R, const double* Qf,
                                     const double* w, int64_t w_batch_stride,
                                     const int32_t* T_star, const int32_t* active,
                                     const double* K, const double* k, const double* alphas,
                                     int32_t n_alpha, int64_t batch, int32_t N, void* workspace,
                                     size_t workspace_bytes, double* X_new, double* U_new,
                                     double* J, double* J_old, int32_t* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_CHAIN_H */
