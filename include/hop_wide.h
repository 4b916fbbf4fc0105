/*
 * hop_wide.h -- the wide entries of libhop_amd.so: fp64 problems with up to 31 states
 * (augmented s = n + 1 <= 32), m <= 16.  The narrow entries of hop.h keep their
 * limits (HOP_MAX_DIM) and their kernels; nothing here changes them, and the ABI
 * version of hop.h covers this header too.
 *
 * Layout conventions, the memory contract, status bits, error codes, streams and hop_last_error are those
 * of hop.h.  Every entry validates its arguments on the host before any launch.
 */
#ifndef HOP_WIDE_H
#define HOP_WIDE_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_WIDE_MAX_DIM 32 /* augmented s = n+1 <= 32 (n <= 31); m stays <= HOP_MAX_DIM */

/*
 * hop_lft_sweep_wide_f64
 * Replaces propagator_all_Jt_aug(A_aug, B_aug, Q_aug, R_list, z0, QT_aug_list,
 *                                T_use, R_inv_cached)
 *   (the reference's horizon_selection.py:36-86), for a batch of independent problems
 *   with 1 <= s <= 32 and 1 <= m <= 16 (HOP_E_SIZE outside), one problem per wave64.
 *
 *   The argument list is hop_lft_sweep_f64's.  R must hold R^-1 (R_inv_cached, or
 *   chol_inv(R_k) per step): r_is_inverse = 0 is HOP_E_ARG.  Element (b,k) block at
 *   R + b*r_batch_stride + k*r_step_stride ([m][m]); shared, per problem or per step.
 *   Every s x s inverse has chol_inv's semantics (utils.py:69-93): symmetrised input,
 *   eps = 1e-9 x10 per failed factorisation up to max_tries, a pivot <= 0 or NaN
 *   rejects, then the LU slot; status bits HOP_ST_JITTER / HOP_ST_LU /
 *   HOP_ST_NONFINITE.  A non-finite block gives NaN at the horizons that read it.
 *   A non-finite z0 row gives that problem NaN at every horizon and HOP_ST_NONFINITE
 *   (t_star = t_min), and changes no other problem.
 *   n_use <= 0 launches nothing; n_use > n_alloc, null pointers and a bad
 *   t_min/t_max window are HOP_E_ARG.
 */
int hop_lft_sweep_wide_f64(const double* A_aug, const double* B_aug, const double* Q_aug,
                           const double* R_inv, int64_t r_batch_stride, int64_t r_step_stride,
                           int32_t r_is_inverse, const double* QT_aug, const double* z0,
                           int64_t z0_batch_stride, int64_t batch, int32_t n_alloc,
                           int32_t n_use, int32_t s, int32_t m, int32_t max_tries,
                           int32_t t_min, int32_t t_max, double* J, int32_t* status,
                           int32_t* t_star, double* j_star, double* dbg_efg,
                           double* dbg_prefix, void* stream);

/*
 * hop_augment_wide_f64
 * Replaces build_augmented_sequence_QR + build_terminal_aug_list
 *   (the reference's augmented.py:10-60 and :63-87), for a batch, 1 <= n <= 31
 *   (s = n + 1 <= 32) and 1 <= m <= 16 (HOP_E_SIZE outside).  The argument list, the
 *   extra stage-cost terms, the wrap mask and the arithmetic are hop_augment_f64's
 *   (the same kernel source with wider LDS tiles); a wrap bit >= n, n_build > n_alloc
 *   and null pointers are HOP_E_ARG, n_build <= 0 launches nothing.
 */
int hop_augment_wide_f64(const double* A, const double* Bm, const double* a_res, const double* X,
                         const double* U, const double* xg, int64_t xg_batch_stride,
                         const double* u_ref, int64_t uref_batch_stride, const double* Q,
                         int64_t q_batch_stride, const double* P, int64_t p_batch_stride,
                         const double* w, int64_t w_batch_stride, const double* qxx_extra,
                         const double* qx_extra, const double* c_extra, uint32_t wrap_mask,
                         double q_reg, double rho_reg, int64_t batch, int32_t n_alloc,
                         int32_t n_build, int32_t n, int32_t m, double* A_aug, double* B_aug,
                         double* Q_aug, double* QT_aug, double* z0, void* stream);

/*
 * hop_riccati_wide_f64
 * Replaces backward_pass_truncated (mode 0, the reference's solver.py:156-230) and
 *   value_expansions_and_gains_prefix (mode 1, its horizon_selection.py:97-212)
 *   for a batch, 1 <= n <= 31 and 1 <= m <= 16 (HOP_E_SIZE outside), one problem per
 *   wave64.  The argument list is hop_riccati_f64's: per-problem horizon and lm, the
 *   extra stage-cost terms, w_stage, the wrap mask, reg_max_tries.  Statuses as
 *   hop_riccati_f64: HOP_ST_JITTER for a chol_solve retry, the LM escalation of mode 1
 *   up to reg_max_tries, HOP_ST_FAIL where the reference raises (mode 0: Quu_reg not
 *   PD without jitter), HOP_ST_NONFINITE with it for non-finite data.  Q_uu stays
 *   m <= 16; only the n-sized objects are wide.  Outputs are written for the steps
 *   below horizon[b] of problems that do not fail.
 */
int hop_riccati_wide_f64(const double* A, const double* Bm, const double* X, const double* U,
                         const double* xg, int64_t xg_batch_stride, const double* u_ref,
                         int64_t uref_batch_stride, const double* Q, int64_t q_batch_stride,
                         const double* R, int64_t r_batch_stride, const double* Qf,
                         int64_t qf_batch_stride, const double* qxx_extra,
                         const double* qx_extra, const double* c_extra, const int32_t* horizon,
                         const double* lm, double w_stage, uint32_t wrap_mask, int32_t mode,
                         int32_t reg_max_tries, int64_t batch, int32_t n_alloc, int32_t n,
                         int32_t m, double* K, double* k, double* Vxx, double* Vx, double* V0,
                         int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_WIDE_H */
