/*
 * hop_fleet.h -- fleets of the built-in systems as device systems of libhop_amd.so:
 * `count` copies of one system of hop.h (0 DI, 1 cart-pole, 2 quadrotor, 3 point mass,
 * 4 segway), stacked member-major and coupled only through the cost.  With these a
 * joint solve of several robots (up to 31 states, 16 inputs) runs end to end on the
 * device.  hop.h, hop_wide.h, hop_wide_jcurve.h, hop_chain.h and hop_onepass.h keep
 * their entries; nothing here changes them, and the ABI version of hop.h covers this
 * header too.
 *
 * The system: x = [x^0 | x^1 | ...] (n = count n_s), u = [u^0 | u^1 | ...]
 *   (m = count m_s), F(x, u) = the concatenation of the members' F(x^j, u^j), each
 *   evaluated by the member's own arithmetic (hop_dynamics_f64's): one fleet step is
 *   bit for bit the members' steps.  Q and Qf are dense n x n, R is dense m x m.
 *
 * Layout conventions, the memory contract (element alignment, written extents, inputs
 * never written), error codes, streams and hop_last_error are those of hop.h.
 * Every entry validates its arguments on the host before any launch:
 *   HOP_E_SIZE (-2)  count < 1, n > HOP_FLEET_MAX_N or m > HOP_FLEET_MAX_M
 *   HOP_E_ARG  (-1)  an unknown system, null pointers, n_use > n_alloc, n_alpha outside
 *                    [1, 8], dt <= 0, negative sizes or strides, a workspace that is too
 *                    small, wrap bits at or above n
 *   0, nothing launched, for batch = 0 (count of rows = 0, n_use = 0).
 * Any batch size and any N are accepted.
 *
 * The argument lists are hop_chain.h's with the fleet's parameters in place of the
 * chain's; the two entries that evaluate the cost take `wrap_mask` (bit i: component i
 * of x - xg and of the line search's dx is an angle, wrapped as in hop.h) after the
 * cost blocks, where the chain has none.
 */
#ifndef HOP_FLEET_H
#define HOP_FLEET_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_FLEET_MAX_N 31 /* states: the wide Riccati pass's limit (a 32-bit wrap mask) */
#define HOP_FLEET_MAX_M 16 /* inputs: the wide Riccati pass's limit */

/* The fleet's parameters: a host struct, read before the launch. */
typedef struct hop_fleet_params {
  int32_t system; /* the member: a system id of hop.h, 0..4 */
  int32_t count;  /* members, >= 1; n = count n_s <= 31, m = count m_s <= 16 */
  double dt;      /* the members' step, > 0 */
} hop_fleet_params;

/*
 * hop_fleet_dynamics_f64
 * One call F(x, u) of the stacked system per row, for `count` rows:
 *   X + r * x_stride [n], U + r * u_stride [m] -> Xn + r * xn_stride [n] (strides in
 *   elements, >= n / m / n).  hop_chain_dynamics_f64's arguments.
 */
int hop_fleet_dynamics_f64(const hop_fleet_params* params, const double* X, int64_t x_stride,
                           const double* U, int64_t u_stride, int64_t count, double* Xn,
                           int64_t xn_stride, void* stream);

/*
 * hop_fleet_rollout_f64
 * Replaces rollout(F, x0, U, max_state_norm) (the reference's solver.py:42-62) on the
 *   stacked state for a batch: x0 [batch or 1][n] (x0_batch_stride 0 = shared),
 *   U [batch][N][m] -> X [batch][N+1][n].  The first state that is not finite in any
 *   member, or whose norm over the whole stacked vector exceeds max_state_norm, and
 *   every state after it are NaN, for every member.
 */
int hop_fleet_rollout_f64(const hop_fleet_params* params, const double* x0,
                          int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                          double max_state_norm, double* X, void* stream);

/*
 * hop_fleet_linearize_f64
 * Replaces linearize_central_diff_traj / linearize_forward_diff_traj and
 *   compute_affine_residuals (the reference's linearization.py:177-270) on the stacked
 *   callable for a batch: X [batch][n_alloc+1][n], U [batch][n_alloc][m] ->
 *   A [batch][n_alloc][n][n], B [batch][n_alloc][n][m] written in full,
 *   a_res [batch][n_alloc][n] = F(x_k, u_k) - x_{k+1} (nullable),
 *   Fx [batch][n_alloc][n] = F(x_k, u_k) (nullable): the layout the augment, sweep and
 *   Riccati entries read.  Steps k < n_use are written, the others are left untouched.
 *   The diagonal blocks are the member's finite-difference columns (hop_linearize_f64's
 *   arithmetic, h = max(eps, rel * max(1, |v|)) with Python's max).  Every off-block
 *   entry is, in the reference, the quotient of two identical numbers: an exact 0.0, or
 *   NaN where that output entry of F is not finite.  The forward form writes an all-NaN
 *   (A_k, B_k) when F(x_k, u_k) is not finite in any member.
 */
int hop_fleet_linearize_f64(const hop_fleet_params* params, const double* X, const double* U,
                            int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                            double epsx, double epsu, double relx, double relu, double* A,
                            double* Bm, double* a_res, double* Fx, void* stream);

/*
 * hop_fleet_cost_true_f64
 * Replaces cost_timeopt_true (the reference's solver.py:65-102) for a batch at the
 *   per-problem horizons T_star [batch], with hop_cost_true_f64's conventions: +inf for
 *   T <= 0 or non-finite data on the rows read, NaN for T > N.  xg [batch or 1][n],
 *   u_ref [batch or 1][m] and w [batch or 1] take a batch stride (0 = shared); Q [n][n],
 *   R [m][m] and Qf [n][n] (the terminal weight, expanded) are dense and shared by the
 *   batch.  No obstacle table.
 */
int hop_fleet_cost_true_f64(const hop_fleet_params* params, const double* X, const double* U,
                            const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                            const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                            const double* R, const double* Qf, const double* w,
                            int64_t w_batch_stride, uint32_t wrap_mask, int64_t batch,
                            int32_t N, double* J, void* stream);

/* bytes of workspace hop_fleet_forward_linesearch_f64 needs (0 for invalid arguments) */
size_t hop_fleet_forward_workspace_bytes(const hop_fleet_params* params, int64_t batch,
                                         int32_t N, int32_t n_alpha);

/*
 * hop_fleet_forward_linesearch_f64
 * Replaces forward_linesearch_fixedT (the reference's solver.py:233-286) on the stacked
 *   callable for a batch, with hop_chain_forward_linesearch_f64's conventions: every
 *   (problem, alpha) pair is rolled out side by side over all N steps (controls
 *   U_k + K_k wrap(dx) + alpha k_k for k < T*, U_k beyond), a non-finite state rejects
 *   that alpha, and the smallest index with J' < J_old strictly wins.  accepted [batch] =
 *   that index, -1 for none, -2 for an inactive problem (active[b] == 0, nullable = all
 *   active; T* outside [0, N]), whose X, U are copied through and whose J is J_old.
 *   K [batch][N][m][n] and k [batch][N][m] as the Riccati entries' mode 0 writes them;
 *   alphas: n_alpha host doubles.  The cost arguments are hop_fleet_cost_true_f64's.  The
 *   rollout arithmetic is hop_fleet_rollout_f64's: with K = 0 and k = 0 the candidate is
 *   X bit for bit.
 */
int hop_fleet_forward_linesearch_f64(const hop_fleet_params* params, const double* X,
                                     const double* U, const double* xg, int64_t xg_batch_stride,
                                     const double* u_ref, int64_t u_ref_batch_stride,
                                     const double* Q, const double* R, const double* Qf,
                                     const double* w, int64_t w_batch_stride, uint32_t wrap_mask,
                                     const int32_t* T_star, const int32_t* active,
                                     const double* K, const double* k, const double* alphas,
                                     int32_t n_alpha, int64_t batch, int32_t N, void* workspace,
                                     size_t workspace_bytes, double* X_new, double* U_new,
                                     double* J, double* J_old, int32_t* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_FLEET_H */
