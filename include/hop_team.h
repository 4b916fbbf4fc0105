/*
 * hop_team.h -- teams: mixed fleets of the built-in systems as device systems of
 * libhop_amd.so.  A team stacks up to 15 members, each one of the systems of hop.h
 * (0 DI, 1 cart-pole, 2 quadrotor, 3 point mass, 4 segway) and each of its own kind and
 * size, member-major, coupled only through the cost.  With these a joint solve of
 * different robots (up to 31 states, 16 inputs) runs end to end on the device.  hop.h,
 * hop_wide.h, hop_wide_jcurve.h, hop_chain.h, hop_onepass.h, hop_fleet.h and
 * hop_fleet_proximity.h keep their entries; nothing here changes them, and the ABI version
 * of hop.h covers this header too.
 *
 * The system: member a owns states [xo_a, xo_a + n_s(a)) and inputs [uo_a, uo_a + m_s(a)),
 *   xo and uo the running sums of the members' sizes in member order; n = sum n_s <= 31,
 *   m = sum m_s <= 16.  F(x, u) = the concatenation of the members' F(x^a, u^a), each
 *   evaluated by the member's own arithmetic (hop_dynamics_f64's) at the shared step dt:
 *   one team step is bit for bit the members' steps.  Q and Qf are dense n x n, R is
 *   dense m x m.  A team of `count` members of one kind is hop_fleet.h's fleet of them,
 *   bit for bit on every output.
 *
 * Layout conventions, the memory contract (element alignment, written extents, inputs
 * never written), error codes, streams and hop_last_error are those of hop.h.
 * Every entry validates its arguments on the host before any launch:
 *   HOP_E_SIZE (-2)  count outside [1, HOP_TEAM_MAX_MEMBERS], n > HOP_FLEET_MAX_N or
 *                    m > HOP_FLEET_MAX_M
 *   HOP_E_ARG  (-1)  an unknown member system, null pointers, n_use > n_alloc, n_alpha
 *                    outside [1, 8], dt <= 0, negative sizes or strides, a workspace that
 *                    is too small, wrap bits at or above n
 *   0, nothing launched, for batch = 0 (count of rows = 0, n_use = 0).
 * Any batch size and any N are accepted.
 *
 * The argument lists are hop_fleet.h's with the team's parameters in place of the
 * fleet's, `wrap_mask` included (bit i: component i of x - xg and of the line search's dx
 * is an angle, wrapped as in hop.h).
 */
#ifndef HOP_TEAM_H
#define HOP_TEAM_H

#include "hop_fleet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_TEAM_MAX_MEMBERS 15 /* n_s >= 2 and n <= 31 */

/* The team's parameters: a host struct, read before the launch. */
typedef struct hop_team_params {
  int32_t count;                        /* members, 1..15 */
  int32_t system[HOP_TEAM_MAX_MEMBERS]; /* member a: a system id of hop.h, 0..4 */
  double dt;                            /* the shared step, > 0 */
} hop_team_params;

/*
 * hop_team_dynamics_f64
 * One call F(x, u) of the stacked system per row, for `count` rows:
 *   X + r * x_stride [n], U + r * u_stride [m] -> Xn + r * xn_stride [n] (strides in
 *   elements, >= n / m / n).  hop_fleet_dynamics_f64's arguments.
 */
int hop_team_dynamics_f64(const hop_team_params* params, const double* X, int64_t x_stride,
                          const double* U, int64_t u_stride, int64_t count, double* Xn,
                          int64_t xn_stride, void* stream);

/*
 * hop_team_rollout_f64
 * Replaces rollout(F, x0, U, max_state_norm) (the reference's solver.py:42-62) on the
 *   stacked state for a batch: x0 [batch or 1][n] (x0_batch_stride 0 = shared),
 *   U [batch][N][m] -> X [batch][N+1][n].  The first state that is not finite in any
 *   member, or whose norm over the whole stacked vector exceeds max_state_norm, and
 *   every state after it are NaN, for every member.
 */
int hop_team_rollout_f64(const hop_team_params* params, const double* x0,
                         int64_t x0_batch_stride, const double* U, int64_t batch, int32_t N,
                         double max_state_norm, double* X, void* stream);

/*
 * hop_team_linearize_f64
 * Replaces linearize_central_diff_traj / linearize_forward_diff_traj and
 *   compute_affine_residuals (the reference's linearization.py:177-270) on the stacked
 *   callable for a batch, with hop_fleet_linearize_f64's layout: A [batch][n_alloc][n][n]
 *   and B [batch][n_alloc][n][m] written in full, a_res and Fx [batch][n_alloc][n]
 *   nullable, steps k < n_use written and the others left untouched.  The diagonal blocks
 *   are the members' finite-difference columns (hop_linearize_f64's arithmetic).  Every
 *   off-block entry is an exact 0.0, or NaN where that output entry of F is not finite
 *   (central); the forward form writes an all-NaN (A_k, B_k) when F(x_k, u_k) is not
 *   finite in any member.
 */
int hop_team_linearize_f64(const hop_team_params* params, const double* X, const double* U,
                           int64_t batch, int32_t n_alloc, int32_t n_use, int32_t central,
                           double epsx, double epsu, double relx, double relu, double* A,
                           double* Bm, double* a_res, double* Fx, void* stream);

/*
 * hop_team_cost_true_f64
 * Replaces cost_timeopt_true (the reference's solver.py:65-102) for a batch at the
 *   per-problem horizons T_star [batch], with hop_fleet_cost_true_f64's conventions: +inf
 *   for T <= 0 or non-finite data on the rows read, NaN for T > N; xg, u_ref and w take a
 *   batch stride (0 = shared); Q [n][n], R [m][m] and Qf [n][n] are dense and shared by
 *   the batch.  No obstacle table.
 */
int hop_team_cost_true_f64(const hop_team_params* params, const double* X, const double* U,
                           const int32_t* T_star, const double* xg, int64_t xg_batch_stride,
                           const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
                           const double* R, const double* Qf, const double* w,
                           int64_t w_batch_stride, uint32_t wrap_mask, int64_t batch,
                           int32_t N, double* J, void* stream);

/* bytes of workspace hop_team_forward_linesearch_f64 needs (0 for invalid arguments) */
size_t hop_team_forward_workspace_bytes(const hop_team_params* params, int64_t batch,
                                        int32_t N, int32_t n_alpha);

/*
 * hop_team_forward_linesearch_f64
 * Replaces forward_linesearch_fixedT (the reference's solver.py:233-286) on the stacked
 *   callable for a batch, with hop_fleet_forward_linesearch_f64's conventions and outputs
 *   (accepted [batch] = the smallest index with J' < J_old strictly, -1 for none, -2 for
 *   an inactive problem, whose X, U are copied through and whose J is J_old).  The cost
 *   arguments are hop_team_cost_true_f64's.  The rollout arithmetic is
 *   hop_team_rollout_f64's: with K = 0 and k = 0 the candidate is X bit for bit.
 */
int hop_team_forward_linesearch_f64(const hop_team_params* params, const double* X,
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
#endif /* HOP_TEAM_H */
