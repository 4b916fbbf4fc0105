/*
 * hop_wide_jcurve.h -- the brute-force J curve of libhop_amd.so for the wide fp64
 * shapes: up to 31 states, m <= 16.  hop.h's hop_bruteforce_jcurve_* keep their limit
 * (HOP_MAX_DIM) and their kernels, hop_wide.h keeps its three entries; nothing here
 * changes them, and the ABI version of hop.h covers this header too.
 *
 * Layout conventions, the memory contract, status bits, error codes, streams and hop_last_error are those
 * of hop.h.  The entry validates its arguments on the host before any launch.
 */
#ifndef HOP_WIDE_JCURVE_H
#define HOP_WIDE_JCURVE_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * hop_bruteforce_jcurve_wide_f64
 * Replaces bruteforce_all_Jt_backward_expansion(A_list, B_list, X, U, xg, u_ref, Q,
 *          R, alpha, w, T_max, lm_lambda, wrap_idx, extra_stage_cost)
 *   (the reference's solver.py:293-358, the select step of
 *   ilqr_timeopt(method="bruteforce")), for a batch, 1 <= n <= 31 and 1 <= m <= 16
 *   (HOP_E_SIZE outside).  The argument list is hop_bruteforce_jcurve_f64's.
 *
 *   J[b][T-1] = V_0 of the length-T value-expansion sweep for T = 1..t_max: the step
 *   of hop_riccati_wide_f64's mode 1 with the fixed lm_lambda and chol_solve's jitter
 *   ladder (no lambda escalation), so a horizon is bit-identical to that pass with
 *   horizon[b] = T and reg_max_tries = 1.  All t_max sweeps of every problem run in
 *   ONE launch: one wave64 per (problem, horizon), a problem's horizons adjacent,
 *   longest first.  No K, k or V array is written.
 *   Outputs: J [batch][t_max]; status [batch][t_max] per horizon (HOP_ST_JITTER for a
 *   chol_solve retry; HOP_ST_FAIL / HOP_ST_NONFINITE where the reference raises
 *   LinAlgError / FloatingPointError, J is NaN there).  As in the reference, only
 *   chol_solve raises: a non-finite x_0 error or a non-finite V_0 leaves inf / NaN in
 *   J without a failure bit.
 *   batch < 0, t_max < 1, t_max > n_alloc (the reference's IndexError), a wrap bit
 *   >= n, a negative stride and a null pointer with batch > 0 are HOP_E_ARG;
 *   batch * t_max waves beyond one grid is HOP_E_SIZE; batch = 0 launches nothing.
 */
int hop_bruteforce_jcurve_wide_f64(const double* A, const double* Bm, const double* X,
                                   const double* U, const double* xg, int64_t xg_batch_stride,
                                   const double* u_ref, int64_t u_ref_batch_stride,
                                   const double* Q, int64_t q_batch_stride, const double* R,
                                   int64_t r_batch_stride, const double* Qf,
                                   int64_t qf_batch_stride, const double* qxx_extra,
                                   const double* qx_extra, const double* c_extra,
                                   double lm_lambda, double w_stage, uint32_t wrap_mask,
                                   int64_t batch, int32_t n_alloc, int32_t n, int32_t m,
                                   int32_t t_max, double* J, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_WIDE_JCURVE_H */
