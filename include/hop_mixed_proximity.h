/*
 * hop_mixed_proximity.h -- the proximity cost of hop_fleet_proximity.h for teams: mixed
 * fleets, whose members are different built-in systems and whose positions therefore
 * differ in dimension.  The cost is evaluated on the device, so that a joint solve of
 * different robots can express "do not collide" without leaving it.  The teams' own header
 * keeps its six functions, hop_fleet_proximity.h its three and hop.h its entries and ABI
 * version; nothing here changes them.
 *
 * The composition is passed flat: `members` (1 .. 15) and `system`, a host array
 *   [members] of system ids (0 double integrator, 1 cart-pole, 2 quadrotor, 3 point mass,
 *   4 segway), stacked member-major as in the teams' header: member a owns states
 *   [xo_a, xo_a + n_s(a)), the offsets being the running sums in member order; n = sum n_s
 *   <= 31 and m = sum m_s <= 16.
 *
 * The cost.  pd_a = the number of position entries of member a, the leading entries of its
 *   state: 1 (DI, cart-pole, segway), 2 (point mass), 3 (quadrotor).  Positions live in a
 *   common workspace of dimension D, the largest pd among the members; member a's
 *   workspace position P_a is its pd_a position entries padded with zeros up to D: a DI
 *   moves on the x axis, a point mass in the plane z = 0, a quadrotor in space.
 *   One bump g(d; r, w) = w exp(-|d|^2 / (2 r^2)), |d|^2 over all D coordinates in
 *   ascending order, is used twice:
 *     obstacles   for every member a and every row (o [D], r, w) of the table:
 *                 g(P_a - o; r, w); the table is [n_obs][D + 2]
 *     separation  for every pair a < b: g(P_a - P_b; sep_radius, sep_weight)
 *   For one bump with value c_i and offset d:
 *     gradient with respect to member a   -(c_i / r^2) d restricted to a's pd_a coordinates
 *                                         (a pair: the second member gets the negative,
 *                                         restricted to its own pd_b)
 *     second-order term                   H = c_i d d^T / r^4, restricted the same way:
 *                                         +H[:pd_a, :pd_a] and +H[:pd_b, :pd_b] on the
 *                                         diagonal position blocks, -H[:pd_a, :pd_b] and its
 *                                         transpose off them
 *   This is J^T H J with selection matrices J, the positive semidefinite part of the bump's
 *   Hessian (see hop_fleet_proximity.h for why the -c_i I / r^2 term is left out, and why Q
 *   needs weight on the position entries).
 *   A team of equal members has D = pd and nothing is padded: it computes the numbers of
 *   the hop_fleet_proximity.h entries bit for bit.
 *
 * Layout conventions, the memory contract of hop.h, error codes, streams and
 * hop_last_error are those of hop_fleet.h.  Every entry validates its arguments on the
 * host before any launch; besides the codes of the plain entries:
 *   HOP_E_SIZE (-2) members outside [1, 15]; n > 31 or m > 16
 *   HOP_E_ARG (-1)  a null `system` or an id outside 0..4; dt not > 0 (the line search);
 *                   and hop_fleet_proximity.h's: a null `prox`, n_obs outside
 *                   [0, HOP_FLEET_MAX_OBSTACLES], a null table with n_obs > 0, a separation
 *                   weight that is negative or not finite, a separation radius that is not
 *                   > 0 (or not finite) where sep_weight > 0
 * The table lives on the device and is not read by the host.  A row of weight 0 and a
 * separation weight of 0 contribute an exact +0.0, whatever their radius.  With n_obs == 0
 * and (sep_weight == 0 or one member) the cost and line-search entries give the plain
 * team's results bit for bit.
 */
#ifndef HOP_MIXED_PROXIMITY_H
#define HOP_MIXED_PROXIMITY_H

#include "hop_fleet_proximity.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * hop_mixed_proximity_taylor_f64
 * The cost and its second-order Taylor terms at `count` stacked states, one per row:
 *   X + r * x_stride [n] (stride in elements, >= n) ->
 *   c [count], cx [count][n], cxx [count][n][n], each nullable.  cx and cxx are written in
 *   full: entries outside the position blocks (a DI's absent y, a point mass's absent z
 *   included) are +0.0.  cxx is symmetric bit for bit.
 */
int hop_mixed_proximity_taylor_f64(int32_t members, const int32_t* system,
                                   const hop_fleet_proximity* prox, const double* X,
                                   int64_t x_stride, int64_t count, double* c, double* cx,
                                   double* cxx, void* stream);

/*
 * hop_mixed_prox_cost_true_f64
 * The team's true cost with the proximity cost: per step acc += (q + r) + w, then
 *   acc += c(x_k) (the reference's order, solver.py:96-99).  The arguments after `system`
 *   are hop_fleet_prox_cost_true_f64's after `params`.
 */
int hop_mixed_prox_cost_true_f64(int32_t members, const int32_t* system, const double* X,
                                 const double* U, const int32_t* T_star, const double* xg,
                                 int64_t xg_batch_stride, const double* u_ref,
                                 int64_t u_ref_batch_stride, const double* Q, const double* R,
                                 const double* Qf, const double* w, int64_t w_batch_stride,
                                 uint32_t wrap_mask, const hop_fleet_proximity* prox,
                                 int64_t batch, int32_t N, double* J, void* stream);

/*
 * hop_mixed_prox_forward_linesearch_f64
 * The team's forward line search at the shared step `dt` with the proximity cost, evaluated
 *   at every candidate's own state (and at X for J_old).  The workspace is the plain team
 *   line search's (its forward_workspace_bytes).
 */
int hop_mixed_prox_forward_linesearch_f64(
    int32_t members, const int32_t* system, double dt, const double* X, const double* U,
    const double* xg, int64_t xg_batch_stride, const double* u_ref, int64_t u_ref_batch_stride,
    const double* Q, const double* R, const double* Qf, const double* w, int64_t w_batch_stride,
    uint32_t wrap_mask, const hop_fleet_proximity* prox, const int32_t* T_star,
    const int32_t* active, const double* K, const double* k, const double* alphas,
    int32_t n_alpha, int64_t batch, int32_t N, void* workspace, size_t workspace_bytes,
    double* X_new, double* U_new, double* J, double* J_old, int32_t* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_MIXED_PROXIMITY_H */
