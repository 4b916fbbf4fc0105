/*
 * hop_testhooks.h -- TEST SUPPORT ONLY.  The two entries below exist so that the test
 * suite can control what a kernel finds in LDS when it starts (LDS keeps its contents
 * from one kernel to the next).  They are not part of the product interface: no caller
 * of libhop_amd.so needs them, hop.h and its ABI version do not cover them, and they may
 * change or go without notice.
 *
 * Return values, hop_last_error and the stream argument are those of hop.h.  Both
 * entries validate their arguments on the host before any launch.
 */
#ifndef HOP_TESTHOOKS_H
#define HOP_TESTHOOKS_H

#include "hop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOP_TEST_LDS_BYTES 163840 /* the LDS of one compute unit */

/*
 * hop_test_lds_fill
 *   Writes the 64-bit `pattern` over the whole LDS of every compute unit.  One
 *   workgroup declares all HOP_TEST_LDS_BYTES statically, so it owns a compute unit's
 *   LDS while it runs; every thread writes the pattern with ordinary LDS stores and the
 *   group then idles for a fixed, bounded number of sleep instructions so that the
 *   dispatcher has to place the other groups on the other compute units.  The grid is
 *   groups_per_cu times the device's compute-unit count (read from the device of
 *   `stream`).
 *   groups_per_cu outside 1 .. 16 is HOP_E_ARG.
 */
int hop_test_lds_fill(uint64_t pattern, int32_t groups_per_cu, void* stream);

/*
 * hop_test_lds_scan
 *   The witness of a fill: `groups` workgroups of `threads` threads with `lds_bytes` of
 *   dynamic LDS each read their allocation without writing it, and all_pattern[group]
 *   (device, int32 [groups]) becomes 1 if every 64-bit word equalled `pattern`, else 0.
 *   Launched with the geometry of a kernel under test it tells whether a fill reached
 *   the LDS that kernel's workgroups get.
 *   lds_bytes outside 8 .. HOP_TEST_LDS_BYTES or no multiple of 8, threads outside
 *   64 .. 1024, groups outside 1 .. 2^31 - 1 and a null all_pattern are HOP_E_ARG.
 */
int hop_test_lds_scan(uint64_t pattern, int32_t lds_bytes, int32_t threads, int64_t groups,
                      int32_t* all_pattern, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOP_TESTHOOKS_H */
