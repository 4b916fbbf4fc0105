/*
 * hop_fleet_proximity.h -- a proximity cost for the fleets of hop_fleet.h: Gaussian bumps
 * that keep the members away from fixed obstacles and from each other, evaluated on the
 * device, so that a joint solve can express "do not collide" without leaving it.
 * hop_fleet.h keeps its seven functions and hop.h its entries and ABI version; nothing
 * here changes them.
 *
 * The cost.  pd = the number of position entries of the member system, the leading
 *   entries of a member's state: 1 (DI, cart-pole, segway), 2 (point mass), 3 (quadrotor).
 *   p_a = member a's position.  One bump g(d; r, w) = w exp(-|d|^2 / (2 r^2)) is used twice:
 *     obstacles   for every member a and every row (o, r, w) of the table: g(p_a - o; r, w)
 *     separation  for every pair a < b: g(p_a - p_b; sep_radius, sep_weight)
 *   For one bump with value c_i and offset d:
 *     gradient with respect to the first point  -(c_i / r^2) d   (a pair: the second point
 *                                                                gets the negative)
 *     Hessian block                             H = c_i d d^T / r^4   (a pair: +H on the two
 *                                                diagonal position blocks, -H on the two
 *                                                off-diagonal ones)
 *   H is the positive semidefinite part of the bump's Hessian: the -c_i I / r^2 term is
 *   left out on purpose (with it the selects' stage blocks Q_k + cxx lose definiteness at
 *   useful weights).  It is therefore NOT the full Hessian of hop_obstacle_cost_f64.
 *   The LFT select inverts Q_k + cxx: a Q that is zero on the position entries makes it
 *   degenerate once a rank-one cxx is added, so give the positions weight.
 *
 * Layout conventions, the memory contract of hop.h, error codes, streams and
 * hop_last_error are those of hop_fleet.h.
 * Every entry validates its arguments on the host before any launch; besides the codes of
 * hop_fleet.h:
 *   HOP_E_ARG (-1)  a null `prox`, n_obs outside [0, HOP_FLEET_MAX_OBSTACLES], a null table
 *                   with n_obs > 0, a separation weight that is negative or not finite, a
 *                   separation radius that is not > 0 (or not finite) where sep_weight > 0
 * The table lives on the device and is not read by the host: its rows are the caller's to
 * check (systems.Proximity does: radius > 0, weight finite and >= 0).  A row of weight 0
 * and a separation weight of 0 contribute an exact +0.0, whatever their radius.
 */
#ifndef HOP_FLEET_PROXIMITY_H
#define HOP_FLEET_PROXIMITY_H

#include "hop_fleet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_FLEET_MAX_OBSTACLES 16 /* rows of the obstacle table */

/* The proximity cost: a host struct, read before the launch. */
typedef struct hop_fleet_proximity {
  const double* obstacles;        /* device, [n_obs][pd + 2]; may be null when n_obs == 0 */
  int32_t n_obs;                  /* 0 .. HOP_FLEET_MAX_OBSTACLES (16) */
  double sep_radius, sep_weight;  /* sep_weight == 0: no separation term */
} hop_fleet_proximity;

/*
 * hop_fleet_proximity_taylor_f64
 * The cost and its second-order Taylor terms at `count` stacked states, one per row:
 *   X + r * x_stride [n] (stride in elements, >= n) ->
 *   c [count], cx [count][n], cxx [count][n][n], each nullable.  cx and cxx are written in
 *   full: entries outside the position blocks are +0.0.  cxx is symmetric bit for bit.
 *   These are the qxx_extra / qx_extra / c_extra of the select and Riccati entries.
 */
int hop_fleet_proximity_taylor_f64(const hop_fleet_params* params,
                                   const hop_fleet_proximity* prox, const double* X,
                                   int64_t x_stride, int64_t count, double* c, double* cx,
                                   double* cxx, void* stream);

/*
 * hop_fleet_prox_cost_true_f64
 * hop_fleet_cost_true_f64 with the proximity cost: per step acc += (q + r) + w, then
 *   acc += c(x_k) (the reference's order, solver.py:96-99).  With n_obs == 0 and
 *   sep_weight == 0 the result is hop_fleet_cost_true_f64's bit for bit.
 */
int hop_fleet_prox_cost_true_f64(const hop_fleet_params* params, const double* X,
                                 const double* U, const int32_t* T_star, const double* xg,
                                 int64_t xg_batch_stride, const double* u_ref,
                                 int64_t u_ref_batch_stride, const double* Q, const double* R,
                                 const double* Qf, const double* w, int64_t w_batch_stride,
                                 uint32_t wrap_mask, const hop_fleet_proximity* prox,
                                 int64_t batch, int32_t N, double* J, void* stream);

/*
 * hop_fleet_prox_forward_linesearch_f64
 * hop_fleet_forward_linesearch_f64 with the proximity cost, evaluated at every candidate's
 *   own state (and at X for J_old).  The workspace is hop_fleet_forward_workspace_bytes'.
 */
int hop_fleet_prox_forward_linesearch_f64(
    const hop_fleet_params* params, const double* X, const double* U, const double* xg,
    int64_t xg_batch_stride, const double* u_ref, int64_t u_ref_batch_stride, const double* Q,
    const double* R, const double* Qf, const double* w, int64_t w_batch_stride,
    uint32_t wrap_mask, const hop_fleet_proximity* prox, const int32_t* T_star,
    const int32_t* active, const double* K, const double* k, const double* alphas,
    int32_t n_alpha, int64_t batch, int32_t N, void* workspace, size_t workspace_bytes,
    double* X_new, double* U_new, double* J, double* J_old, int32_t* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_FLEET_PROXIMITY_H */
