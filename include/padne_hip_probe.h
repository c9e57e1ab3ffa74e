/* padne_hip_probe.h -- TEST-ONLY probes of libpadne_hip.so.  Neither the drop-in boundary (include/padne_hip.h) nor the
 * multi-rank scaffolding (include/padne_hip_test.h): nine entries.  padne_test_product drives a single product launcher of the
 * solver on inputs a test chooses, so that every SpMV / SpMM kernel form and epilogue can be held against a host reference;
 * padne_test_kkt_state copies one device array of a padne_kkt plan out, so that every stage of the plan can;
 * padne_test_amg_state copies out what a level of the multigrid hierarchy decided in its setup, padne_test_amg_tail hands
 * out the gathered operator of a row-partitioned hierarchy; padne_test_halo_exchange and padne_test_amg_apply_dist run one
 * halo exchange and one cycle of a row-partitioned hierarchy on a test's vector; padne_test_pool_guard reads the counters of
 * the device allocator's guarded mode and runs its self-test; padne_test_scan runs one exclusive scan, in any of its host
 * forms, on counts a test chooses, and padne_test_csr_op one transpose or sparse product of the multigrid setup on matrices a
 * test chooses, so that the sparse primitives under the assembly and the setup can be held against host references at their
 * own limits.  Bound by padne_amd/_hip.py (PROBE_SIGNATURES). */
#ifndef PADNE_HIP_PROBE_H
#define PADNE_HIP_PROBE_H

#include "padne_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ONE product in one of the call shapes the solver uses (spmv.hip / spmm.hip: launch_spmv, launch_spmm), for checking every kernel
 * form and epilogue against a host reference (tests/test_products_vs_reference.py).  The entries are the solver's own: nothing is
 * instantiated here.
 *
 * First the matrix is prepared by the library's builders, as `flags` asks (in this order): PADNE_TEST_HIERARCHY marks it a
 * multigrid operator (eligible for a wave per row, no x-window plan), then 1/diag, the single-precision copies, the x-window plan,
 * the wide plan, the interior / boundary split of its first n_owned columns (built although no exchange runs beside it).
 *
 * A launcher ID names a call shape: the types, the epilogue and the operands the solver passes.  The flat arguments map onto the
 * operands by role (ProductArgs, padne_amd/csrc/common.hpp): aux0 = x_pre, aux1 = b, aux2 = dinv, and the rest by name.  Device
 * pointers; unused ones may be null; the float shapes take (float)scale.
 *   SPMV_MODE / SPMV_PART        double, `mode` (, part): x, y, b, dinv, scale, dot_with, partials
 *   SPMV_DOT_X32                 SPMV_DOT with x stored in float, y in double: partials
 *   SPMV_F32 / SPMV_F32_PART     float, `mode` (, part): x, y, b, dinv, scale, partials
 *   SPMV_F32_RESTRICT            SPMV_RESTRICT: r = x, b_c = y, x_c = y2, dinv_c = aux2, c = scale
 *   SPMV_F32_RESID_PRE           SPMV_RESID_PRE: b = x, resid = y, dinv = aux2, c = scale
 *   SPMV_F32_EXIT / _EXIT_PART   the exit stage, SPMV_JACOBI: x, y (double) or z32 = y2, b, dinv, scale, dot_with, partials,
 *                                out_scale2 (, part)
 *   SPMV_F32_WUP                 SPMV_WUP: e = x, x_out = y, x_pre = aux0, r_pre = b = aux1, dinv = aux2, scale
 *   SPMV_F32_WUP_EXIT            the same as an exit stage: z = y (double) or z32 = y2, dot_with, partials, out_scale2, rhs
 *   SPMM_MODE / SPMM_F32         as SPMV_MODE / SPMV_F32 on [n][k] vectors (k, mode)
 *   SPMM_F32_EXIT                as SPMV_F32_EXIT (y32 = y2), out_scale2[k]
 *   SPMM_F32_WUP / _WUP_EXIT     as SPMV_F32_WUP / _WUP_EXIT, rhs = the fine level's right-hand side [n][k]
 *
 * With partials_host != null the launch gets a partial-sum slot of k (SpMM) or 1 rows of kMaxPartials = 2048 doubles, filled
 * with the sentinel 0xff bytes before the launch and copied to partials_host afterwards, all of it (n_partials_host >= rows * 2048).
 * info[8] receives: the kernel form the launch took (PADNE_TEST_FORM_*; the SpMM kernel counts as a tile form), xw_state,
 * xw_run, xw_nruns, the number of partial sums per row (spmv_partials / spmm8_grid), the interior and boundary tile counts of
 * the split plan, and where the boundary launch's partial sums start. */
enum {
    PADNE_TEST_SPMV_MODE = 0, PADNE_TEST_SPMV_PART = 1, PADNE_TEST_SPMV_DOT_X32 = 2, PADNE_TEST_SPMV_F32 = 3,
    PADNE_TEST_SPMV_F32_PART = 4, PADNE_TEST_SPMV_F32_RESTRICT = 5, PADNE_TEST_SPMV_F32_RESID_PRE = 6,
    PADNE_TEST_SPMV_F32_EXIT = 7, PADNE_TEST_SPMV_F32_EXIT_PART = 8, PADNE_TEST_SPMV_F32_WUP = 9,
    PADNE_TEST_SPMV_F32_WUP_EXIT = 10, PADNE_TEST_SPMM_MODE = 11, PADNE_TEST_SPMM_F32 = 12, PADNE_TEST_SPMM_F32_EXIT = 13,
    PADNE_TEST_SPMM_F32_WUP = 14, PADNE_TEST_SPMM_F32_WUP_EXIT = 15
};
enum { PADNE_TEST_HIERARCHY = 1, PADNE_TEST_DINV = 2, PADNE_TEST_F32 = 4, PADNE_TEST_XW = 8, PADNE_TEST_XW_WIDE = 16,
       PADNE_TEST_SPLIT = 32 };
enum { PADNE_TEST_FORM_NONE = 0, PADNE_TEST_FORM_WPR = 1, PADNE_TEST_FORM_LIST = 2, PADNE_TEST_FORM_LONG = 3,
       PADNE_TEST_FORM_WIDE = 4, PADNE_TEST_FORM_TILE = 5 };
int padne_test_product(padne_ctx *ctx, padne_csr *m, int32_t flags, int64_t n_owned, int32_t launcher, int32_t mode,
                       int32_t k, int32_t part, const void *x, void *y, void *y2, const void *aux0, const void *aux1,
                       const void *aux2, const void *rhs, const double *dot_with, const int32_t *done_flag, double scale,
                       const double *out_scale2, double *partials_host, int64_t n_partials_host, int32_t *info);

/* ONE device array of a padne_kkt plan, copied to out_host as it lies on the device (tests/test_kkt_plan_vs_reference.py).
 * Read-only: the entry waits for the context's stream, copies, and changes nothing.
 *   IMAP     int32[N]                           reduced unknown of every unknown, -1 = none
 *   SRC_OF   int32[n_free]                      the unknown whose row opens the sum of reduced row t
 *   B, Y     double[(n_cols + n_extra) n_free]  right-hand sides and solutions of the reduced system, column after column
 *   C        double[N width]                    known part of the potentials, in the products' layout (kkt.hip, "blocks of
 *                                               right-hand sides"); only when the last stage 1 had known potentials, and not
 *                                               after a stage 2 that used the array for the caller's layout (every n_cols
 *                                               but 1, 2, 4 and 8, where the two layouts coincide)
 *   V        double[N width]                    the potentials in the products' layout: of stage 1, or final after stage 2
 *   Z        double[n_extra N]                  expanded solutions of the extra right-hand sides
 * with n_cols, n_extra of the last stage 1 and width = the doubles per row of its products' layout (n_cols / 8 full groups of
 * 8, the rest widened to 1, 2, 4 or 8).  PADNE_E_INVALID when n_bytes is not the size of the array, or the array does not
 * exist yet: B .. Z before the first completed stage 1, C as said. */
enum { PADNE_TEST_KKT_IMAP = 0, PADNE_TEST_KKT_SRC_OF = 1, PADNE_TEST_KKT_B = 2, PADNE_TEST_KKT_Y = 3, PADNE_TEST_KKT_C = 4,
       PADNE_TEST_KKT_V = 5, PADNE_TEST_KKT_Z = 6 };
int padne_test_kkt_state(const padne_kkt *plan, int32_t which, void *out_host, int64_t n_bytes);

/* What level `level` of the multigrid hierarchy of `m` decided in its setup, copied to out_host
 * (tests/test_amg_vs_reference.py).  Read-only: the entry waits for the context's stream, copies, and changes nothing; it
 * does not build a hierarchy that is not there.
 *   AGG      int32[n_l]   aggregate (column of P_l) of every vertex of the level
 *   ROOT     int8[n_l]    1 where the independent-set rounds made the vertex a root
 *   SCALARS  double[4]    lambda (the bound of D^-1 A the smoother uses), jac (its damping), 1.0 if the level has a fused
 *                         up-leg operator W, 1.0 if the cycle runs in single precision
 *   EXPORT   int32[n_export]  row-partitioned levels: the owned vertices of the level whose values the other ranks read,
 *                         in the order of this rank's exchange segment
 *   HALO     int64[4]     row-partitioned levels: m (length of every rank's exchange segment on this level), n_export, and
 *                         of the hierarchy: rows of the gathered tail, first gathered row of this rank's piece
 * AGG and ROOT exist only on levels that were coarsened by a setup that ran under PADNE_AMG_KEEP=1 (the switch makes the
 * setup copy them out of its scratch; without it nothing is kept).  On a row-partitioned level they describe the rank's own
 * block: n_l owned vertices, aggregates numbered within the rank.  PADNE_E_INVALID when n_bytes is not the size of the
 * array, the array was not kept, the level does not exist, or EXPORT / HALO are asked of a single-GPU hierarchy. */
enum { PADNE_TEST_AMG_AGG = 0, PADNE_TEST_AMG_ROOT = 1, PADNE_TEST_AMG_SCALARS = 2, PADNE_TEST_AMG_EXPORT = 3,
       PADNE_TEST_AMG_HALO = 4 };
int padne_test_amg_state(padne_ctx *ctx, const padne_csr *m, int32_t level, int32_t which, void *out_host, int64_t n_bytes);

/* The gathered operator of the row-partitioned hierarchy of `m` -- the last partitioned level with the rows of all ranks, in
 * rank order, which every rank holds and coarsens further on its own -- as a BORROWED handle: valid while `m` lives, never to
 * be destroyed by the caller.  padne_csr_to_host, padne_amg_level, padne_test_amg_state and padne_amg_apply work on it as on
 * any single-GPU matrix.  PADNE_E_INVALID when `m` has no row-partitioned hierarchy. */
int padne_test_amg_tail(const padne_csr *m, const padne_csr **tail);

/* ONE halo exchange of the caller's vector through the context's plan (padne_ctx_set_halo): x_host[n_owned] is uploaded
 * (as_float: converted to float first), halo_exchange_plan / halo_exchange_plan_f32 runs once, and the whole vector comes
 * back, out_host[n_owned + world * m] (as_float: widened again).  The exchange area is filled with 0xff bytes before the
 * exchange, so a slot in which nothing arrives reads as NaN; slots behind a rank's n_export are padding and undefined.
 * Collective: every rank of the team or communicator calls it.  Waits for the context's stream. */
int padne_test_halo_exchange(padne_ctx *ctx, int32_t as_float, const double *x_host, double *out_host);

/* padne_amg_apply for this rank's rows of a row-partitioned matrix, n_owned x (n_owned + world * m) under the context's halo
 * plan: builds the hierarchy over all ranks if needed and runs ONE cycle, r_host[n_owned] -> z_host[n_owned], with the
 * partial-sum slot and the null unit of padne_amg_apply.  Collective.  Waits for the context's stream. */
int padne_test_amg_apply_dist(padne_ctx *ctx, padne_csr *a, const double *r_host, double *z_host);

/* The guarded mode of the context's device allocator, PADNE_POOL_GUARD=<hex fill byte> (INTEGRATION.md;
 * tests/test_device_memory.py): every block handed out lies between two guard zones that are compared with their canary when
 * the block is freed, and its bytes are filled with the fill byte first.  Counters of the context plus its second stream's.
 *   op 0  copy the counters out
 *   op 1  reset them, then as op 0
 *   op 2  the self-test (PADNE_E_INVALID without the switch): two blocks of 1000 bytes; the first is read back, then eight
 *         bytes are copied from the host to offset 1000 of the first and to offset -8 of the second -- inside their guard
 *         zones, which belong to the blocks' own allocations -- and both are freed: two violations.  Then as op 0.
 * out[8]: guarded blocks handed out; violations; of the first violation the requested bytes, the side (1 in front of the
 * block, 2 behind it) and the offset of the first changed byte from the block's start (negative in front); side and offset of
 * the last violation; and in out[7] the fill byte (-1: mode off), or after op 2 whether every byte read back was the fill
 * byte (1 / 0).  A violation is only ever counted: nothing aborts. */
int padne_test_pool_guard(padne_ctx *ctx, int32_t op, int64_t *out);

/* ONE exclusive scan of int32 counts (assemble.hip; tests/test_sparse_primitives_vs_reference.py), through the library's own
 * host forms: nothing is instantiated here.  in_host[n] is uploaded to a device buffer that starts `misalign` (0 to 3) int32
 * elements behind a 16-byte boundary; `out` (n + 1 elements) lies at the same offset of a buffer of its own, filled with 0xff
 * bytes first, or with in_place != 0 is the input buffer itself.  The scan runs in the form asked for and out[0 .. n] is copied
 * to out_host.
 *   PLAIN     exclusive_scan_i32: info[1] = the total where the form reports one (PADNE_OK, PADNE_E_TOOLARGE), else -1;
 *             info[2] = -1
 *   FLAGGED   exclusive_scan_i32_flagged: info[1] = the total, info[2] = the negative flag
 *   ASYNC     exclusive_scan_i32_async (nothing read back): info[1] = info[2] = -1
 *   HALVES    scan_i32_begin / scan_i32_end with the total wanted: info[1], info[2] = what scan_i32_end handed out
 * info[0] = the return code of the form.  The entry itself returns PADNE_OK whenever the probe worked, whatever the scan
 * returned; PADNE_E_INVALID for an unknown form, a misalignment outside 0 .. 3, or in_place with n > 32768 (in == out is
 * documented for the one-workgroup kernel only).  Waits for the context's stream. */
enum { PADNE_TEST_SCAN_PLAIN = 0, PADNE_TEST_SCAN_FLAGGED = 1, PADNE_TEST_SCAN_ASYNC = 2, PADNE_TEST_SCAN_HALVES = 3 };
int padne_test_scan(padne_ctx *ctx, int32_t form, int64_t n, const int32_t *in_host, int32_t misalign, int32_t in_place,
                    int32_t *out_host, int64_t *info);

/* ONE transpose or sparse product of the multigrid setup (amg.hip: transpose, spgemm) on the caller's matrices, as a new
 * matrix the caller destroys (tests/test_sparse_primitives_vs_reference.py).  The setup's own entries: nothing is
 * instantiated here.
 *   TRANSPOSE      out = X^T               (Y, Z unused)
 *   MATMUL         out = X Y               (Z unused); a sum that is exactly zero is not stored
 *   MATMUL_CHAIN   out = X (Y Z), with Y Z left in its merge slots and read from there by the second product, as the setup
 *                  forms R (A P); Y Z comes back as a matrix, and is read as one, only where its product had to be split
 * PADNE_E_INVALID when the shapes do not chain.  Waits for the context's stream. */
enum { PADNE_TEST_CSR_TRANSPOSE = 0, PADNE_TEST_CSR_MATMUL = 1, PADNE_TEST_CSR_MATMUL_CHAIN = 2 };
int padne_test_csr_op(padne_ctx *ctx, int32_t op, const padne_csr *X, const padne_csr *Y, const padne_csr *Z, padne_csr **out);

#ifdef __cplusplus
}
#endif

#endif /* PADNE_HIP_PROBE_H */
