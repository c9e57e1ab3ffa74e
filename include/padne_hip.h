/*
 * padne_hip.h -- C ABI of libpadne_hip.so, the MI355X (gfx950) implementation of
 * the padne solver hot path.
 *
 * The reference (atx/padne) has no FFI for this path: the seam is the Python
 * module padne/solver.py.  Each entry point below names the reference code whose
 * arithmetic it replaces (file:line in the reference tree); INTEGRATION.md shows
 * the ctypes stub a padne maintainer would add to call them.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PADNE_E_* code on failure;
 *     padne_last_error() returns a thread-local human readable message.
 *     Nothing throws across the boundary.
 *   - "host" pointers are caller-owned host memory; "dev" pointers are raw device
 *     addresses (hipMalloc / torch tensor.data_ptr()) valid on the context's GPU.
 *   - all calls are blocking unless the name ends in _async.
 *   - indices are int32 inside a matrix (nnz < 2^31), sizes are int64.
 *   - all floating point data that crosses this boundary is IEEE binary64 (solver.py:21, DTYPE = float64), and so are
 *     assembly, the solver's own products, residuals and dot products; only the multigrid V-cycle INSIDE the
 *     preconditioner runs on single-precision copies of its operators (it has to be a fixed SPD operator, not an
 *     accurate one; PADNE_AMG_F64=1 keeps it in binary64).
 */
#ifndef PADNE_HIP_H
#define PADNE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PADNE_ABI_VERSION 1

#define PADNE_OK            0
#define PADNE_E_INVALID    -1   /* bad argument (null pointer, negative size, index out of range) */
#define PADNE_E_HIP        -2   /* a HIP runtime call failed */
#define PADNE_E_NOMEM      -3
#define PADNE_E_NONMANIFOLD -4  /* triangle soup is not an oriented manifold (mesh.py:342-343 ValueError) */
#define PADNE_E_NOTCONVERGED -5 /* PCG hit max_iter (solution still returned) */
#define PADNE_E_COMM       -6   /* RCCL not available / communicator failure */
#define PADNE_E_BREAKDOWN  -7   /* PCG breakdown: matrix not SPD (p.Ap <= 0) or NaN */
#define PADNE_E_TOOLARGE   -8   /* a count exceeds the 32-bit index space of the CSR structures (nnz, slot offsets) */
#define PADNE_E_NOCOARSEN  -9   /* multigrid setup: the aggregation no longer shrinks the operator.  Internal to the
                                   solve (which then preconditions with the diagonal, info.levels = 0); returned only by
                                   the entry points that expose the hierarchy itself (padne_amg_apply, padne_amg_level) */

typedef struct padne_ctx padne_ctx;   /* device, stream, workspaces, optional RCCL communicator */
typedef struct padne_csr padne_csr;   /* device-resident CSR matrix (f64 values, i32 indices)  */
typedef struct padne_kkt padne_kkt;   /* device-resident plan of solve_system for one assembled system */
typedef struct padne_refine padne_refine;     /* device-resident result of one refinement round */
typedef struct padne_polymesh padne_polymesh; /* device-resident meshes of one batch of polygons */
typedef struct padne_sampler padne_sampler;   /* device-resident meshes, potentials and point-location index of a solved board */

/* ---- library / context ------------------------------------------------------------------- */
int         padne_abi_version(void);
const char *padne_last_error(void);
/* number of visible GPUs, or a negative error code */
int         padne_device_count(void);
/* create a context on `device` with its own non-blocking stream */
int         padne_ctx_create(int device, padne_ctx **out);
int         padne_ctx_destroy(padne_ctx *ctx);
int         padne_ctx_synchronize(padne_ctx *ctx);
/* raw hipStream_t of the context (for event timing by the caller) */
void       *padne_ctx_stream(padne_ctx *ctx);

/* ---- multi-GPU (RCCL over xGMI; one process per GPU) --------------------------------------
 * No reference counterpart: the reference is single-process.
 * padne_comm_unique_id fills 128 bytes on one rank; the caller broadcasts them
 * (torch.distributed) and every rank calls padne_ctx_comm_init. */
int padne_comm_unique_id(void *id128);
int padne_ctx_comm_init(padne_ctx *ctx, const void *id128, int rank, int world_size);
int padne_ctx_comm_rank(padne_ctx *ctx, int *rank, int *world_size);
/* communication this process has issued since the library was loaded: calls[0..2] / bytes[0..2] = the COLLECTIVES
 * all-reduce (f64 scalars), all-gather of f64 values, all-gather of f32 values; calls[3] / bytes[3] = peer-to-peer halo
 * exchanges (every rank stores its exported values into the other ranks' mailboxes: no collective).  Bytes are this
 * rank's contributions.  Bookkeeping for DESIGN.md section 6 (what a multi-GPU solve costs), also counted for the
 * in-process team. */
int padne_comm_call_counts(long long calls[4], long long bytes[4]);
/* kernels and asynchronous fills this process has queued through the library since it was loaded (all contexts).  What a
 * solve costs in LAUNCHES is read off the difference around it: below a million unknowns per GPU a solve is bound by its
 * launches, not by bytes (bench.py: rank_proxy). */
int padne_launch_count(long long *count);
/* The same collectives through a transport of the CALLER (gloo, MPI, ...) instead of RCCL: ranks RCCL cannot connect
 * -- two processes on one GPU -- or a host that has no RCCL.  `allgather(user, send, recv, bytes_per_rank)` gathers
 * bytes_per_rank bytes of HOST memory from every rank into recv (rank order; send may lie inside recv) and returns 0;
 * any other value fails the call that needed it with PADNE_E_COMM.  Every collective of the library then goes device ->
 * host -> callback -> device (sums are formed in rank order: the same bits on every rank, as with RCCL); it is the
 * slow path by construction -- what makes it usable is the peer-to-peer halo exchange below, which takes the four
 * exchanges of a CG iteration out of the collectives. */
typedef int (*padne_allgather_fn)(void *user, const void *send, void *recv, int64_t bytes_per_rank);
int padne_ctx_comm_init_host(padne_ctx *ctx, int rank, int world_size, padne_allgather_fn allgather, void *user);
/* Peer-to-peer halo exchange between PROCESSES (one per GPU, or several on one GPU): every rank owns a mailbox in
 * device memory -- a ring of exchange entries of world_size * slots_per_rank 8-byte cells behind a page of arrival
 * flags -- allocated uncached and shared through hipIpc.  A halo exchange is then: every rank STORES its exported
 * values straight into every rank's mailbox and, when its stores are out (system-scope release), writes the exchange's
 * sequence number into its flag there; the receiver's next kernel on the stream waits for the flags of all senders
 * (bounded: PADNE_P2P_TIMEOUT_MS, default 20 s, then the solve returns PADNE_E_COMM) and copies the entry behind its
 * owned values.  No collective, no host involvement, and the interior tiles of the product the exchange is for run
 * while the stores travel.  Protocol, collective over the ranks of a communicator (RCCL or host):
 *   padne_ctx_p2p_export   allocate this rank's mailbox, write its 64-byte hipIpc handle to handle64
 *   -- the caller all-gathers the handles (rank order) --
 *   padne_ctx_p2p_import   open the other ranks' mailboxes (handles = world_size * 64 bytes); from here on exchanges
 *                          whose plan has at most slots_per_rank slots per rank go peer to peer
 *   padne_ctx_p2p_selftest one real exchange of known values through the mailboxes (2 s bound): *ok = 1 if every rank's
 *                          stores and flags arrived here -- the caller gathers the verdicts and closes unless all say yes
 *   padne_ctx_p2p_close    back to the all-gather (also done by padne_ctx_destroy); collective like the ones above
 * PADNE_NO_P2P=1 keeps the all-gather although mailboxes exist (A/B, tests). */
int padne_ctx_p2p_export(padne_ctx *ctx, int32_t slots_per_rank, void *handle64);
int padne_ctx_p2p_import(padne_ctx *ctx, const void *handles, int32_t n_handles);
int padne_ctx_p2p_selftest(padne_ctx *ctx, int32_t *ok);
int padne_ctx_p2p_close(padne_ctx *ctx);

/* Halo plan of a row-partitioned matrix (layer partition).  Every vector the
 * local matrix multiplies is laid out [n_owned owned entries | world_size * m exchanged entries];
 * before each product the rank copies its `n_export` values export_idx[k] (local indices) into its
 * own segment and one ncclAllGather (m doubles per rank) fills the rest, so a column that refers to
 * unknown export_idx[k] of rank r is column n_owned + r*m + k.  The local matrix therefore has
 * n_owned + world_size*m columns and its first n_owned rows are the owned equations (further rows
 * must be empty).  With a communicator set, all PCG dot products are summed over the ranks by
 * ncclAllReduce on the context stream.  n_owned < 0 clears the plan. */
int padne_ctx_set_halo(padne_ctx *ctx, int64_t n_owned, int32_t m, int32_t n_export,
                       const int32_t *export_idx_host);

/* ---- device memory helpers (thin, so that callers need no HIP binding of their own) -------- */
int padne_dev_alloc(padne_ctx *ctx, int64_t bytes, void **dev_out);
int padne_dev_free(padne_ctx *ctx, void *dev);
int padne_dev_upload(padne_ctx *ctx, void *dev_dst, const void *host_src, int64_t bytes);
int padne_dev_download(padne_ctx *ctx, void *host_dst, const void *dev_src, int64_t bytes);
int padne_dev_memset(padne_ctx *ctx, void *dev, int value, int64_t bytes);

/* ---- matrices ------------------------------------------------------------------------------ */
/* upload a host CSR (scipy layout: int32 indptr[n_rows+1], int32 indices[nnz], f64 data[nnz]).
 * Replaces L.tocsc() as the hand-off of the assembled system, solver.py:772.
 * The columns of a row need not ascend and a row may name a column more than once (scipy's canonical form does neither; the
 * layout does not forbid it).  Such a matrix MEANS the matrix its entries sum to, as a non-canonical scipy csr_matrix does,
 * and is STORED as that matrix in canonical form: the upload sorts every row by column and adds the parts of a repeated
 * column in the order of their position (on the host, in the one pass that also checks the index range; a sum that comes to
 * 0.0 stays a stored entry, as in scipy's sum_duplicates).  Every entry that takes the handle therefore sees unique, strictly
 * ascending columns, and padne_csr_shape / padne_csr_to_host report the canonical arrays and their nnz, which is smaller than
 * indptr[n_rows] when a column was repeated.  A canonical matrix is uploaded from the caller's arrays as they stand. */
int padne_csr_from_host(padne_ctx *ctx, int64_t n_rows, int64_t n_cols,
                        const int32_t *indptr, const int32_t *indices, const double *data,
                        padne_csr **out);
int padne_csr_destroy(padne_csr *m);
int padne_csr_shape(const padne_csr *m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
/* copy back to caller-allocated host arrays (sizes from padne_csr_shape) */
int padne_csr_to_host(padne_ctx *ctx, const padne_csr *m, int32_t *indptr, int32_t *indices, double *data);

/* Assemble the global system matrix L in the reference layout and sign.
 *   mesh part  : HalfEdge.cotan (mesh.py:124-139), laplace_operator (solver.py:171-213),
 *                process_mesh_laplace_operators (solver.py:563-575)
 *   lumped part: the COO stamps produced by stamp_network_into_system / setup_ground_node
 *                (solver.py:469-560), already in global indices, in stamp order.
 * xy[n_vert][2], tri[n_tri][3] hold mesh-LOCAL vertex ids; mesh m owns vertices
 * [mesh_vertex_offset[m], mesh_vertex_offset[m+1]) (VertexIndexer, solver.py:221-229) and
 * triangles [mesh_tri_offset[m], mesh_tri_offset[m+1]).  Duplicate (row, col) stamps are summed
 * in stamp order after the mesh contribution; exact zeros are not stored (solver.py:187-190).
 * Returns PADNE_E_NONMANIFOLD where Mesh.from_triangle_soup raises ValueError (mesh.py:342-343).
 * The matrix arrays are allocated for an upper bound of the entries (one per triangle corner, two per vertex, the
 * stamps) and the rows are written once, in place; padne_csr_shape reports the exact count.  PADNE_E_TOOLARGE when
 * that bound exceeds the 32-bit index space of a CSR matrix (about 268 M mesh vertices).  The single-pass row kernel
 * finds its offsets with a scan that runs inside it and whose waits are bounded; on a chip shared with other work such a
 * wait can run out -- the rows are then built again in two passes (lengths, scan, fill: the same bits, about three times
 * the time), never an error of the call. */
int padne_assemble_system(padne_ctx *ctx, int64_t n_unknowns,
                          int64_t n_vert, const double *xy_host,
                          int64_t n_tri, const int32_t *tri_host,
                          int64_t n_mesh, const int64_t *mesh_vertex_offset,
                          const int64_t *mesh_tri_offset, const double *conductance,
                          int64_t n_coo, const int64_t *coo_row, const int64_t *coo_col,
                          const double *coo_val,
                          padne_csr **out);
/* Structured test / benchmark mesh generated on the device (no reference counterpart: it stands where the CGAL mesher
 * stands, padne/mesh.py:662-795, for the synthetic configs of SURVEY.md section 8d): nx * ny vertices spaced h from
 * (origin_x, origin_y), row-major, interior vertices displaced by U(-jitter h, +jitter h), cells split by alternating
 * diagonals into counter-clockwise triangles.  The displacements are output 2 v + 1 and 2 v + 2 of numpy's PCG64
 * stream whose 128-bit state and increment are pcg64_state_inc[0..3] = state hi, state lo, inc hi, inc lo
 * (default_rng(seed).bit_generator.state), so the arrays equal padne_amd.synthetic.jittered_grid bit for bit.
 * xy_dev: 2 nx ny doubles, tri_dev: 6 (nx-1)(ny-1) int32, both device memory (padne_dev_alloc). */
int padne_generate_grid_mesh(padne_ctx *ctx, int64_t nx, int64_t ny, double h, double jitter, double origin_x,
                             double origin_y, const uint64_t *pcg64_state_inc, void *xy_dev, void *tri_dev);

/* The same for ONE RANK'S PIECE of a mesh that is partitioned across GPUs (flags bit 0): the triangles are those that
 * touch a vertex the rank owns, so the vertices of the ring around the owned region have incomplete fans and the
 * manifold test (PADNE_E_NONMANIFOLD) is switched off -- the rows of ring vertices are dropped by the caller
 * (padne_csr_relabel); validate the whole mesh on one rank instead.  flags = 0 is padne_assemble_system.
 * With either entry point `xy_host` / `tri_host` may also be DEVICE pointers (e.g. filled by padne_generate_grid_mesh):
 * the kernels then read the caller's arrays, the copy the matrix keeps for padne_csr_power_density is made device to device
 * on the context's second stream beside them, and nothing crosses PCIe (the arrays must stay valid until the call returns). */
int padne_assemble_system_ex(padne_ctx *ctx, int64_t n_unknowns, int64_t n_vert, const double *xy_host,
                             int64_t n_tri, const int32_t *tri_host, int64_t n_mesh,
                             const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                             const double *conductance, int64_t n_coo, const int64_t *coo_row,
                             const int64_t *coo_col, const double *coo_val, int32_t flags, padne_csr **out);

/* out = scale * P^T M P restricted to kept indices: entry (i,j,v) of M becomes
 * (map[i], map[j], scale*v) if both maps are >= 0; duplicates are summed.  Used to turn the
 * reference's indefinite KKT system into the SPD system A = -L_vv on the free potentials
 * (ground eliminated, voltage-source-tied nodes merged; DESIGN.md "reduction"). */
int padne_csr_reduce(padne_ctx *ctx, const padne_csr *m, const int32_t *map_host,
                     int64_t n_out, double scale, padne_csr **out);
/* Rectangular form of the same operation with separate row and column maps (row_map has m.n_rows entries,
 * col_map m.n_cols): out (n_rows_out x n_cols_out) = scale * R^T M C.  The row-partitioned solve uses it
 * to keep exactly the owned rows of a rank while the columns keep the exchange slots (DESIGN.md
 * "multi-GPU"). */
int padne_csr_relabel(padne_ctx *ctx, const padne_csr *m, const int32_t *row_map_host, int64_t n_rows_out,
                      const int32_t *col_map_host, int64_t n_cols_out, double scale, padne_csr **out);
/* rows of `top` followed by the rows of `bottom` (equal column counts) */
int padne_csr_vstack(padne_ctx *ctx, const padne_csr *top, const padne_csr *bottom, padne_csr **out);

/* ---- SpMV ---------------------------------------------------------------------------------- */
/* y = M x, host vectors (the reference's residual product L_csc @ v, solver.py:775) */
int padne_spmv(padne_ctx *ctx, const padne_csr *m, const double *x_host, double *y_host);
/* y = M x on device vectors, enqueued `repeat` times on the context stream; blocking at the end */
int padne_spmv_dev(padne_ctx *ctx, const padne_csr *m, const void *x_dev, void *y_dev, int repeat);
/* Y = M X for 8 right-hand sides at once, device arrays interleaved as X[i*8 + j] = entry i of vector j
 * (X: n_cols x 8, Y: n_rows x 8); every column of Y is bit-identical to padne_spmv_dev on that vector.
 * The batched solve (padne_solve_spd with n_rhs a multiple of 8) is built on it. */
int padne_spmm8_dev(padne_ctx *ctx, const padne_csr *m, const void *x_dev, void *y_dev, int repeat);
/* residual: returns ||M x - b||_2 (device), host vectors in */
int padne_residual_norm(padne_ctx *ctx, const padne_csr *m, const double *x_host,
                        const double *b_host, double *norm_out);

/* ---- solve --------------------------------------------------------------------------------- */
typedef struct padne_solve_opts {
    double  rtol;        /* stop when ||b - A x||_2 <= max(rtol*||b||_2, atol); if the TRUE residual
                            stagnates above that (binary64 evaluation floor of b - A x, ~1e-12 at
                            N = 5 M) the solve ends successfully within 10x of the request and
                            reports what it reached in padne_solve_info.rel_residual           */
    double  atol;
    int32_t max_iter;    /* iterations allowed per right-hand side (a lockstep group: per group), restarts included;
                            exact, whatever check_every.  A solve that ends there above its tolerance returns
                            iterate number max_iter with PADNE_E_NOTCONVERGED: reaching the limit is not a failure
                            of the multigrid preconditioner, nothing is redone with Jacobi (0 = 100000)         */
    int32_t precond;     /* 0 = Jacobi, 1 = smoothed-aggregation multigrid V-cycle (the hierarchy is built on
                            first use and cached on the matrix; the cycle runs in single precision inside
                            the double-precision CG unless PADNE_AMG_F64 is set.  The single-precision cycle is
                            handed r / ||b|| rounded to single precision, and its last product forms r.z with
                            that rounded residual: alpha and beta are textbook PCG's to single rounding, 2^-24
                            relative, not to double rounding; x, r and p.Ap are double throughout.  On a row-partitioned
                            matrix it is one hierarchy over all ranks, or block-Jacobi with
                            padne_csr_set_preconditioner_block)                                    */
    int32_t check_every; /* iterations enqueued between host convergence polls (0 = auto); kernels queued behind the
                            iteration that stops return at once: iterations, restarts and every bit of x are the
                            same for any value                                                                  */
    int32_t flags;       /* bit0: x holds an initial guess (otherwise x0 = 0)
                            bit1: time sampled SpMV launches with HIP events -> info.spmv_seconds
                            bit2: rebuild everything derived from the matrix inside this call (multigrid
                                  hierarchy, single-precision copies, x-window plan of the SpMV)   */
} padne_solve_opts;

typedef struct padne_solve_info {
    int32_t iterations;      /* summed over the right-hand sides; in a lockstep group every column counts its own
                                steps until it has converged (a zero right-hand side: none)                     */
    int32_t restarts;        /* true-residual restarts taken                     */
    double  rel_residual;    /* final TRUE ||b - A x|| / ||b||                    */
    double  abs_residual;    /* final TRUE ||b - A x||; both: the largest over the right-hand sides */
    double  solve_seconds;   /* device time of the iteration loop (HIP events)    */
    double  spmv_seconds;    /* average device time of one SpMV launch (flags bit1) */
    int32_t status;          /* PADNE_OK / PADNE_E_NOTCONVERGED / PADNE_E_BREAKDOWN */
    int32_t n_rhs;
    double  precond_setup_seconds; /* device time of the multigrid setup done inside this call (0 if cached) */
    double  operator_complexity;   /* sum of nnz over the levels / nnz of the fine matrix                    */
    int32_t levels;                /* multigrid levels (0 with Jacobi)                                       */
    int32_t precond_fallbacks;     /* right-hand sides redone with Jacobi after a multigrid breakdown/stall
                                      (not after max_iter iterations: see padne_solve_opts.max_iter)         */
} padne_solve_info;

/* Preconditioned CG on an SPD CSR matrix: replaces scipy.sparse.linalg.spsolve in
 * solve_system (solver.py:773) once the system is reduced.  b, x: host f64[n_rhs][n]
 * (row-major, one right-hand side after another).  With the multigrid preconditioner on one GPU, groups of
 * 8 right-hand sides (remainders of 5-7 zero-padded to 8, a remainder of exactly 4 in a group of width 4) advance in
 * lockstep: one pass over the matrix and the hierarchy per iteration for the whole group; results do not depend on the
 * grouping beyond the tolerance.  PADNE_E_NOTCONVERGED still returns the best iterate in x and the residual reached in info. */
int padne_solve_spd(padne_ctx *ctx, const padne_csr *a, const double *b_host, double *x_host,
                    int32_t n_rhs, const padne_solve_opts *opts, padne_solve_info *info);
/* same with device-resident b and x */
int padne_solve_spd_dev(padne_ctx *ctx, const padne_csr *a, const void *b_dev, void *x_dev,
                        int32_t n_rhs, const padne_solve_opts *opts, padne_solve_info *info);

/* ---- solve_system as a whole (solver.py:767-780: L.tocsc(), spsolve, residual) ---------------------------------------
 * The reference hands the indefinite KKT matrix (multiplier rows of voltage sources / regulators / the ground,
 * solver.py:493-538, 544-560) to SuperLU.  Here it is reduced to the SPD system A y = b on the free potentials
 *  and a padne_kkt plan keeps that reduction on the device: the index map, A = -P^T L P with its
 * multigrid hierarchy, and the N-vectors r, v.  The host describes the reduction by O(#constraints) lists:
 *   elim_sorted[n_elim]   potentials without a reduced unknown of their own, ascending: potentials known outright (the
 *                         ground, nodes tied to it by sources, pins of floating copper) and the members of source-tied
 *                         groups other than the group's representative;
 *   tied_member / tied_rep[n_tied]  those members (ascending) and the representative they are numbered through;
 *   index_map_host        optional int32[N] (NULL: built on the device as  i - #{e in elim : e < i}): a map the caller
 *                         made itself; n_free = number of reduced unknowns.
 *   flags                 bit 0: number the reduced unknowns by horizontal strips of the meshes `L` was assembled from
 *                         (mesh, strip of about three vertex spacings, x; unknowns that are no vertex behind them) -- the
 *                         band numbering the SpMV's x windows need when the mesher numbered the vertices in insertion
 *                         order (CGAL).  Internal to the plan: r and v keep the caller's numbering.  Needs a matrix from
 *                         padne_assemble_system (it carries its mesh); PADNE_E_INVALID if the keys do not fit
 *                         (>= 65535 meshes, > 65535 strips in a mesh): the caller may then pass its own map.
 * `L` is borrowed and must outlive the plan. */
int padne_kkt_create(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int64_t n_elim,
                     const int64_t *elim_sorted, int64_t n_tied, const int64_t *tied_member, const int64_t *tied_rep,
                     const int32_t *index_map_host, int64_t n_free, int32_t flags, padne_kkt **out);
int padne_kkt_destroy(padne_kkt *plan);
/* borrowed handle of the reduced SPD matrix (for introspection; do not destroy) */
int padne_kkt_matrix(const padne_kkt *plan, const padne_csr **reduced_out);
/* Stage 1 of a solve.  r_host[N]: the right-hand side (solver.py:757-760, 478-541), uploaded ONCE and in parallel with the
 * multigrid setup of A (built on the first call and kept with the plan; opts.flags bit 2 rebuilds it).
 * known_idx / known_val: the known part c of the potentials (v = c + P y): non-zero only on members of constraint groups.
 * Extra right-hand sides k = 0..n_extra-1 (regulator gain columns gamma_k, solver.py:537-538) as sparse columns in
 * ORIGINAL row indices, CSR-like: entries extra_ptr[k]..extra_ptr[k+1] of extra_row / extra_val; b_k = P^T gamma_k.
 * The device forms b = -P^T (r - L c), solves A y = b and A z_k = b_k (zero right-hand sides are skipped; the relative
 * tolerance is tightened so that ||b - A y|| <= abs_residual_target where opts.rtol ||b|| would be looser: the reference's
 * absolute residual bar, tests/test_solver.py:2083-2089; 0 = off), expands v = c + P y and Z_k = P z_k, and returns
 * probe_out[(1 + n_extra)][n_probe]: rho = r - L v, then L Z_k, at the probed unknowns (the members of the constraint
 * groups) -- what the host needs to peel the multiplier currents from.  v stays on the device.
 * At most 4095 extra right-hand sides (with r itself, the 4096 padne_kkt_solve_block allows).
 * Returns PADNE_E_NOTCONVERGED like padne_solve_spd (the iterate is kept, padne_kkt_finish may follow). */
int padne_kkt_solve(padne_ctx *ctx, padne_kkt *plan, const double *r_host, int64_t n_known, const int64_t *known_idx,
                    const double *known_val, int32_t n_extra, const int64_t *extra_ptr, const int64_t *extra_row,
                    const double *extra_val, int64_t n_probe, const int64_t *probe_idx, double *probe_out,
                    const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info);
/* Stage 2: v += sum_k extra_coeff[k] Z_k (regulator currents), v[mult_idx] = mult_val (the recovered multiplier
 * currents: sources, regulators, ground row), then residual_norm = ||L v - r||_2 on the ORIGINAL system
 * (solver.py:775) while v[N] travels to v_host -- its only crossing of PCIe. */
int padne_kkt_finish(padne_ctx *ctx, padne_kkt *plan, int32_t n_extra, const double *extra_coeff, int64_t n_mult,
                     const int64_t *mult_idx, const double *mult_val, double *v_host, double *residual_norm_out);
/* Stage 1 for a block of n_cols right-hand sides (the reference's spsolve with a 2-D r): r_host[N][n_cols] row-major, uploaded
 * once in that layout; known_val[n_cols][n_known] (one index list for all columns: the union, zero where a column knows
 * nothing); the extra right-hand sides as in padne_kkt_solve, solved ONCE for the whole block.  The products with L take one
 * pass over L per group of up to 8 columns; all n_cols + n_extra reduced columns (at most 4096) go through
 * padne_solve_spd_dev together, so its lockstep grouping sees them all (zero columns are skipped and come back as zeros).
 * probe_out[n_cols + n_extra][n_probe]: rho_j = r_j - L v_j for every column, then L Z_k.  padne_kkt_solve is the case
 * n_cols = 1. */
int padne_kkt_solve_block(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, const double *r_host, int64_t n_known,
                          const int64_t *known_idx, const double *known_val, int32_t n_extra, const int64_t *extra_ptr,
                          const int64_t *extra_row, const double *extra_val, int64_t n_probe, const int64_t *probe_idx,
                          double *probe_out, const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info);
/* Stage 2 of a block: v_j += sum_k extra_coeff[j][k] Z_k, v_j[mult_idx] = mult_val[j][:], then residual_norms_out[j] =
 * ||L v_j - r_j||_2 while V travels to v_host[N][n_cols] (row-major, the layout r_host had).  n_cols and n_extra as in
 * the stage 1 before it; padne_kkt_finish is the case n_cols = 1. */
int padne_kkt_finish_block(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int32_t n_extra, const double *extra_coeff,
                           int64_t n_mult, const int64_t *mult_idx, const double *mult_val, double *v_host,
                           double *residual_norms_out);
/* padne_kkt_solve_block with the block given as n_entries COO triples (r_row[e], r_col[e], r_val[e]) instead of a dense
 * r_host: the plan's r block is zeroed on the device and the triples scattered into it, in the same [N][n_cols] layout;
 * everything after that is padne_kkt_solve_block.  Load cases of one board: only the source terminals and the multiplier
 * rows are non-zero.  Duplicate or out-of-range (row, column) pairs: PADNE_E_INVALID before the device is touched. */
int padne_kkt_solve_block_coo(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int64_t n_entries, const int64_t *r_row,
                              const int32_t *r_col, const double *r_val, int64_t n_known, const int64_t *known_idx,
                              const double *known_val, int32_t n_extra, const int64_t *extra_ptr, const int64_t *extra_row,
                              const double *extra_val, int64_t n_probe, const int64_t *probe_idx, double *probe_out,
                              const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info);
/* padne_kkt_solve_block with the block r_dev[N][n_cols] (row-major) already on the device, on the context's stream: one
 * device-to-device copy into the plan's r takes the place of the upload, everything after that is padne_kkt_solve_block and
 * gives its bits for the same block.  The caller keeps r_dev; it is read before the call returns. */
int padne_kkt_solve_block_dev(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, const void *r_dev, int64_t n_known,
                              const int64_t *known_idx, const double *known_val, int32_t n_extra, const int64_t *extra_ptr,
                              const int64_t *extra_row, const double *extra_val, int64_t n_probe, const int64_t *probe_idx,
                              double *probe_out, const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info);
/* Per-face sigma |grad V|^2 of every column of the block the last padne_kkt_finish_block left on the device, over the mesh
 * `L` keeps: out_host[n_cols][n_tri] row-major, column j bit-identical to padne_csr_power_density on V[:, j].  Nothing
 * crosses PCIe but the result.  PADNE_E_INVALID when no block has been finished since the last solve, when n_cols is not
 * that block's, or when `L` carries no mesh. */
int padne_kkt_power_density_block(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, double *out_host);
/* Element cases: from the block V[N][n_cols] the last padne_kkt_finish_block left on the device, form V'[N][n_out] with
 * V'[i][c] = sum over the entries e = w_ptr[c] .. w_ptr[c + 1] - 1 of row c, in that order, of w_val[e] * V[i][w_col[e]]
 * (CSR weights, one row per output column).  The first product starts the sum and no product is fused with its addition,
 * so a row of one entry with coefficient 1.0 copies the column's bits; a row without entries gives zeros.  V' becomes the
 * block the plan holds, as if padne_kkt_finish_block had left it with n_out columns: padne_kkt_power_density_block,
 * padne_kkt_current_cases, padne_kkt_error_estimate and the others then work on it unchanged (and a further
 * padne_kkt_combine_block combines V').  V' also goes to v_host[N][n_out] if that is not null.  Out of place: V and V'
 * are on the device together, (n_cols + n_out) * N * 8 bytes.  No atomics: two calls give the same bits.  Preconditions
 * and errors as padne_kkt_power_density_block; PADNE_E_INVALID also unless 1 <= n_out <= 4096, w_ptr[0] = 0 and w_ptr is
 * monotone, the columns of every row are strictly ascending and in [0, n_cols), and every coefficient is finite. */
int padne_kkt_combine_block(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int32_t n_out, const int64_t *w_ptr,
                            const int32_t *w_col, const double *w_val, double *v_host);
/* Adjoint sensitivities over the mesh `L` keeps, from the block the last padne_kkt_finish_block left on the device: column 0
 * of V is the solution x, the other columns are the solutions the adjoints are combined from.  Adjoint j is
 * lambda_j = sum_m weights[j][m] V[:, m] (weights[n_obj][n_cols] row-major; a selection when L is symmetric, the Woodbury
 * combination when regulators make it unsymmetric), formed per face in registers, never as an N-vector.  Per face f, with
 * the assembly's cot weights w_ik = |cot|/2 of the corner opposite edge (i,k) and the sheet conductance sigma of its mesh,
 * s_j,f = sigma sum_{edges of f} w_ik (lambda_j,i - lambda_j,k)(x_i - x_k) = sigma dJ_j / dsigma_f.  Writes
 * power_out[n_tri] (column 0's sigma |grad V|^2, bit-identical to padne_csr_power_density on V[:, 0]),
 * density_out[n_obj][n_tri] = s_j,f / area_f and mesh_total_out[n_obj][n_mesh] = the sum of s_j,f over each mesh, summed
 * in a fixed order (no floating-point atomics: two calls give the same bits).  Preconditions and errors as
 * padne_kkt_power_density_block; 1 <= n_obj <= 4096 and finite weights, else PADNE_E_INVALID. */
int padne_kkt_sensitivity_block(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int32_t n_obj, const double *weights,
                                double *power_out, double *density_out, double *mesh_total_out);
/* Currents over the mesh `L` keeps, from column 0 of the block the last padne_kkt_finish_block left on the device (a block
 * of any width: padne_kkt_current_cases below with one reported column, without its envelope and its power).  Per face
 * t, with the face gradient of padne_csr_power_density and the sheet conductance sigma of its mesh: J_out[n_tri][2] =
 * -sigma grad V (so |J|^2 / sigma is the power density) and mag_out[n_tri] = |J|; per mesh m, mesh_max_out[m] = the
 * largest |J| of its faces and mesh_face_out[m] = that face (global index, the lowest on a tie; -1.0 and -1 for a mesh
 * without faces).  Cut c is the directed segment cut_xy[c] = (start x, y, end x, y) on the meshes m with
 * mesh_layer[m] == cut_layer[c]; cut_out[c] = sum over the face edges (P, Q) (P the lower global vertex) that cross it of
 * sigma |cot|/2 (V_left - V_right), where an edge crosses when orient(start, end, .) > 0 differs between P and Q and
 * orient(P, Q, .) > 0 differs between start and end (orient(a, b, p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x);
 * left: orient(start, end, .) > 0).  Everything is summed in a fixed order: two calls give the same bits.  Preconditions
 * and errors as padne_kkt_sensitivity_block; n_tri and n_mesh must be the mesh's, 0 <= n_cut <= 4096, end points finite
 * and start != end, else PADNE_E_INVALID. */
int padne_kkt_current_report(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int64_t n_tri, int32_t n_mesh,
                             const int32_t *mesh_layer, int32_t n_cut, const int32_t *cut_layer, const double *cut_xy,
                             double *J_out, double *mag_out, double *mesh_max_out, int64_t *mesh_face_out, double *cut_out);
/* padne_kkt_current_report for every column j of the block the last padne_kkt_finish_block left on the device (load cases),
 * and the envelope over the columns: the two entries are one function and one set of kernels.  Column-major results: J_out[n_cols][n_tri][2], mag_out[n_cols][n_tri],
 * mesh_max_out / mesh_face_out[n_cols][n_mesh], cut_out[n_cols][n_cut]; row 0 of each holds the bits padne_kkt_current_report
 * gives (any n_cols >= 1).  mesh_power_out[n_cols][n_mesh] = per mesh the sum over its faces of sigma sum_{edges} w_ik
 * (V_i - V_k)^2 with the assembly's |cot|/2 weights: for column 0 the bits of padne_kkt_sensitivity_block's mesh_total_out
 * with one objective of weight 1 on a one-column block.  env_out[n_tri] = max_j |J_j| per face and env_case_out[n_tri] the
 * lowest column that attains it: the columns are visited in order from column 0 and a later one replaces the value only
 * when strictly greater, so a face whose |J| is NaN in column 0 keeps NaN and case 0.  J_out and mag_out may both be null
 * ("envelope only"): then no per-column field is written on the device or copied home; every other result is the same.
 * env_out and env_case_out may both be null likewise: then no envelope is computed.
 * Everything is summed in a fixed order: two calls give the same bits.  Preconditions and errors as
 * padne_kkt_current_report. */
int padne_kkt_current_cases(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int64_t n_tri, int32_t n_mesh,
                            const int32_t *mesh_layer, int32_t n_cut, const int32_t *cut_layer, const double *cut_xy,
                            double *J_out, double *mag_out, double *env_out, int32_t *env_case_out, double *mesh_max_out,
                            int64_t *mesh_face_out, double *mesh_power_out, double *cut_out);
/* Gradient-recovery (Zienkiewicz-Zhu) estimate of the discretisation error over the mesh `L` keeps, from column 0 of the
 * block the last padne_kkt_finish_block left on the device.  Per face f (corners in the order of padne_csr_power_density):
 * g_f its gradient, A_f its area.  G_out[n_vert][2] = (sum A_f g_f) / (sum A_f) over the faces incident to each vertex, added
 * in ascending global face number (0 for a vertex without faces or whose areas sum to zero; no special case on the
 * boundary).  eta_out[n_tri] = sqrt(sigma (A_f / 3) (|m_12|^2 + |m_23|^2 + |m_31|^2)) with d_c = G_(corner c) - g_f and
 * m_ab = (d_a + d_b) / 2: sigma times the integral over f of |G_h - g_f|^2 for the piecewise-linear G_h, in watts under the
 * root.  Per mesh m: mesh_error_out[m] = sum eta_f^2, mesh_power_out[m] = sum sigma A_f |g_f|^2, mesh_max_out[m] = the
 * largest eta_f and mesh_face_out[m] its face (global index, the lowest on a tie; -1.0 and -1 for a mesh without faces).
 * The vertex -> faces lists are built on the first call and kept with the plan.  Everything is summed in a fixed order:
 * two calls give the same bits.  Preconditions and errors as padne_kkt_current_report; n_tri, n_vert and n_mesh must be the
 * mesh's, else PADNE_E_INVALID. */
int padne_kkt_error_estimate(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int64_t n_tri, int64_t n_vert, int32_t n_mesh,
                             double *G_out, double *eta_out, double *mesh_error_out, double *mesh_power_out,
                             double *mesh_max_out, int64_t *mesh_face_out);
/* Goal-oriented (dual-weighted) error estimate over the mesh `L` keeps, from the block the last padne_kkt_finish_block left
 * on the device.  Field 0 is column 0 of V, field 1 + j the adjoint lambda_j = sum_m weights[j][m] V[:, m] of objective j
 * (weights[n_obj][n_cols] as padne_kkt_sensitivity_block takes them).  Every field a goes through the passes of
 * padne_kkt_error_estimate: g_f^a, G_v^a, d_c^a = G^a_(corner c) - g_f^a, m_12^a = (d_1^a + d_2^a) / 2 (likewise m_23, m_31),
 * eta_f^a.  Field 0's results (G_out .. mesh_face_out) are padne_kkt_error_estimate's, bit for bit, and power_out[n_tri] is
 * column 0's sigma |grad V|^2, bit-identical to padne_csr_power_density on V[:, 0].  Per objective j and face
 * f: dual_eta_out[n_obj][n_tri] = eta_f^(1+j); delta_out[n_obj][n_tri] = sigma (A_f / 3) (m_12^0 . m_12^(1+j) + m_23^0 .
 * m_23^(1+j) + m_31^0 . m_31^(1+j)), signed: sigma times the integral over f of the product of the two recovered-minus-raw
 * gradient fields; omega_out[n_obj][n_tri] = eta_f^0 eta_f^(1+j) >= |delta|.  Per objective and mesh:
 * mesh_omega_out / mesh_delta_out[n_obj][n_mesh] = the sums over the mesh's faces, mesh_top_out[n_obj][n_mesh] = the
 * largest omega and mesh_top_face_out its face (global index, the lowest on a tie; -1.0 and -1 for a mesh without faces).
 * Objectives are processed 8 per launch.  The vertex -> faces lists are those of padne_kkt_error_estimate, built by the
 * first call of either and kept with the plan.  Everything is summed in a fixed order: two calls give the same bits.
 * Preconditions and errors as padne_kkt_sensitivity_block and padne_kkt_error_estimate. */
int padne_kkt_goal_error(padne_ctx *ctx, padne_kkt *plan, int32_t n_cols, int32_t n_obj, const double *weights, int64_t n_tri,
                         int64_t n_vert, int32_t n_mesh, double *power_out, double *G_out, double *eta_out,
                         double *mesh_error_out, double *mesh_power_out, double *mesh_max_out, int64_t *mesh_face_out, double *dual_eta_out,
                         double *delta_out, double *omega_out, double *mesh_omega_out, double *mesh_delta_out,
                         double *mesh_top_out, int64_t *mesh_top_face_out);

/* Row-partitioned runs, optional: attach the rank's owned x owned diagonal block; with precond = 1 the
 * multigrid hierarchy is then built on that block only (block-Jacobi with multigrid blocks, no
 * communication inside the cycle, 3-6x more CG iterations than the default hierarchy over all ranks).
 * Borrowed handle; null detaches. */
int padne_csr_set_preconditioner_block(padne_csr *a, padne_csr *block);

/* z = M^-1 r: one V-cycle of the multigrid preconditioner (built on first use and cached on `a`);
 * host vectors.  Exposed for tests: M must be symmetric positive definite for PCG to apply. */
int padne_amg_apply(padne_ctx *ctx, padne_csr *a, const double *r_host, double *z_host);
/* The same for the cycle the lockstep groups run: k = 2, 4 or 8 right-hand sides r_host[k][n] (one after the other) through
 * the batched single-precision cycle in one pass, column j in units of sqrt(unit2_host[j]) (0: as it is) as the lockstep
 * loop hands it ||b_j||^2; z_host[k][n].  PADNE_E_INVALID where the hierarchy has no batched cycle (double precision, one
 * level).  Exposed for tests. */
int padne_amg_apply_batch(padne_ctx *ctx, padne_csr *a, int32_t k, const double *r_host, const double *unit2_host,
                          double *z_host);

/* introspection: borrowed handle of a hierarchy operator (which: 0 = A_l, 1 = P_l, 2 = R_l = P_l^T);
 * it stays valid as long as `a` does and must NOT be destroyed */
int padne_amg_level(padne_ctx *ctx, padne_csr *a, int level, int which, const padne_csr **out);

/* ---- connection snapping ------------------------------------------------------------------- */
/* index of the nearest point of xy[n_points][2] for every query point (squared Euclidean distance in binary64,
 * ties to the smallest index): what NodeIndexer.create asks of its per-layer KD-trees
 * (_construct_kdtrees solver.py:356-396, query solver.py:425).  Brute force on the device: at a million vertices
 * the KD-tree build is two thirds of the host time of solve(). */
int padne_nearest_vertex(padne_ctx *ctx, int64_t n_points, const double *xy_host, int64_t n_query,
                         const double *query_host, int64_t *index_out_host);
/* The same, and for every query the number of points at EXACTLY the minimum distance (tie_count_out_host, >= 1).  The
 * reference's KD-tree (solver.py:389-392, query :425) returns whichever of several equidistant vertices its traversal meets
 * first; a caller that wants the reference's choice re-resolves the queries with a count above 1 with that tree (they are
 * rare: a connection exactly between vertices of an unjittered grid) -- NodeIndexer.create does. */
int padne_nearest_vertex_ties(padne_ctx *ctx, int64_t n_points, const double *xy_host, int64_t n_query,
                              const double *query_host, int64_t *index_out_host, int32_t *tie_count_out_host);

/* ---- post-processing ----------------------------------------------------------------------- */
/* per-face power density  p = sigma*|grad V|^2 with the reference's barycentric difference
 * quotient (compute_triangle_gradient solver.py:689-725, compute_power_density :728-745).
 * Also performs the scatter of produce_layer_solutions (solver.py:596-598): `potential` is the
 * global solution vector, vertex v of mesh m reads potential[mesh_vertex_offset[m] + v]. */
int padne_power_density(padne_ctx *ctx, int64_t n_vert, const double *xy_host,
                        int64_t n_tri, const int32_t *tri_host,
                        int64_t n_mesh, const int64_t *mesh_vertex_offset,
                        const int64_t *mesh_tri_offset, const double *conductance,
                        const double *potential_host, double *power_out_host);

/* The same power densities for the mesh an assembled system was built from: padne_assemble_system leaves the mesh
 * on the device with the matrix, so only the potentials travel (n_vert doubles up, n_tri doubles down).
 * potential_host: the first n_vert entries of the solution in the global vertex numbering. */
int padne_csr_power_density(padne_ctx *ctx, const padne_csr *m, const double *potential_host, double *power_out_host);

/* per-face gradient of the linear interpolant of `potential` (compute_triangle_gradient,
 * solver.py:689-725), faces visited as (v3, v1, v2) like Face.vertices (mesh.py:320-325) */
int padne_face_gradient(padne_ctx *ctx, int64_t n_vert, const double *xy_host,
                        int64_t n_tri, const int32_t *tri_host,
                        int64_t n_mesh, const int64_t *mesh_vertex_offset,
                        const int64_t *mesh_tri_offset, const double *potential_host,
                        double *gx_out_host, double *gy_out_host);

/* padne_kkt_error_estimate for meshes and potentials given from the host (arguments as padne_power_density, at least one
 * mesh): the same passes, the vertex -> faces lists built for this call alone. */
int padne_error_estimate(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                         int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                         const double *conductance, const double *potential_host, double *G_out, double *eta_out,
                         double *mesh_error_out, double *mesh_power_out, double *mesh_max_out, int64_t *mesh_face_out);

/* padne_kkt_goal_error for meshes and fields given from the host: potential_host[n_vert][n_fields] row-major holds
 * n_fields >= 2 (at most 4097) potentials per vertex, field 0 is paired with each of the other n_fields - 1, which take the
 * place of the adjoints (n_obj = n_fields - 1 in the shapes of the outputs).  The other arguments are
 * padne_error_estimate's, and so are the field-0 results, bit for bit; power_out[n_tri] has the bits of padne_power_density. */
int padne_goal_error(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                     int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                     const double *conductance, int32_t n_fields, const double *potential_host, double *power_out,
                     double *G_out, double *eta_out, double *mesh_error_out, double *mesh_power_out, double *mesh_max_out,
                     int64_t *mesh_face_out, double *dual_eta_out, double *delta_out, double *omega_out,
                     double *mesh_omega_out, double *mesh_delta_out, double *mesh_top_out, int64_t *mesh_top_face_out);

/* ---- refinement: conforming refined meshes from one flag per face -----------------------------
 * No reference counterpart.  4-triangle longest-edge refinement with conforming closure ("Refinement") of a batch
 * of meshes given as padne_power_density takes them, flag_host[n_tri] != 0 for the faces to refine.  Edges are the distinct
 * keys lo * n_vert + hi over the global vertex numbers of the corners (tri[f][c], tri[f][(c + 1) % 3]), numbered in
 * ascending key order; d_e = dx * dx + dy * dy from lo to hi; a face's longest edge has the greatest d_e, the lowest edge
 * number on a tie.  Every edge of a flagged face is marked, then the longest edge of every face with a marked edge, until
 * nothing changes.  One new vertex 0.5 * (p[lo] + p[hi]) per marked edge, behind the old vertices of its mesh in ascending
 * edge number; old vertices keep index and coordinates.  With the face rotated so that its longest edge is (a, b), c
 * opposite, m, p, q the midpoints of ab, bc, ca: an unmarked face is copied; otherwise (a, m, q), (q, m, c) if ca is marked
 * else (a, m, c), then (m, b, p), (m, p, c) if bc is marked else (m, b, c).  Children lie in parent order.
 * The sizes of the result are known only afterwards, so it stays on the device behind a handle (destroyed before its
 * context): new_vertex_count_out[n_mesh] and new_face_count_out[n_mesh] size the arrays of padne_refine_fetch;
 * counts_out[4] (may be null) = edges of the batch, edges marked by the flags, edges marked after the closure, closure
 * sweeps queued.  PADNE_E_INVALID for a triangle index out of range and a face that names a vertex twice,
 * PADNE_E_NONMANIFOLD for an edge with more than two faces or with two faces that run it in the same direction.  Two calls
 * give the same bits. */
int padne_refine_create(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                        int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                        const uint8_t *flag_host, int64_t *new_vertex_count_out, int64_t *new_face_count_out,
                        int64_t *counts_out, padne_refine **out);
/* xy_out[sum of the vertex counts][2]; tri_out[sum of the face counts][3] and parent_out[...] with mesh-local vertex and
 * parent-face indices; ends_out[new vertices][2] the mesh-local (lo, hi) ends of the edge every new vertex halves, mesh by
 * mesh in the order of the new vertices. */
int padne_refine_fetch(padne_ctx *ctx, const padne_refine *r, double *xy_out, int32_t *tri_out, int32_t *parent_out,
                       int32_t *ends_out);
int padne_refine_destroy(padne_refine *r);     /* NULL is accepted */

/* ---- grid mesher: first meshes of polygons with holes ------------------------------------------
 * Stands where the reference's CGAL mesher stands (padne/mesh.py:662-795); not a replacement for it: isosurface stuffing on
 * a uniform lattice of spacing h whose lines sit at global multiples of h ("Grid mesher"; the rules, expression
 * by expression, at the top of csrc/polymesh.hip).  One call meshes a batch: polygon p has the rings
 * poly_ring_ptr[p] .. poly_ring_ptr[p + 1] (the exterior first, then the holes; orientation does not matter under the
 * even-odd rule), ring r the vertices ring_ptr[r] .. ring_ptr[r + 1] of ring_xy[..][2], without a closing duplicate.
 * snap in (0, 1/2): a lattice vertex with a cut closer than snap * |edge| moves onto the boundary.
 * The sizes of the result are known only afterwards, so it stays on the device behind a handle (destroyed before its
 * context): vertex_count_out[n_poly] and face_count_out[n_poly] size the arrays of padne_polymesh_fetch.  The arrays may
 * stay on the device: padne_polymesh_arrays hands out their device addresses (xy double[..][2], tri and kind int32, laid out
 * as padne_polymesh_fetch returns them, valid until the handle is destroyed), which is what an assembly that takes mesh
 * arrays already on the device (padne_assemble_system_ex) reads.
 * Limits: a lattice (bounding box plus one cell on every side) of at most 2^24 vertices, a batch of at most 2^27 lattice
 * vertices, fewer than 2^31 (segment, cell row) pairs; beyond them PADNE_E_INVALID.  PADNE_E_INVALID also for a ring with
 * fewer than 3 vertices, a polygon without a ring, a coordinate that is not finite, h <= 0, snap outside (0, 1/2) and a
 * null pointer.  Two calls give the same bits. */
int padne_polymesh_create(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                          const double *ring_xy, double h, double snap, int64_t *vertex_count_out, int64_t *face_count_out,
                          padne_polymesh **out);
/* The same, graded: fine at the boundary and at the seeds, coarse inside ("Graded grid mesher").  Lattice, sign,
 * cuts and snap as above; then, in integers only:
 *   plain     a cell (ci, cj) of the lattice's (nx - 1) x (ny - 1) cells is plain when its four corners are inside and not
 *             snapped; seed k makes the cell (floor(x / h) - i0, floor(y / h) - j0) of every polygon of the batch not plain
 *             when that polygon's lattice has it (i0, j0: the global index of the lattice's first line); cells outside the
 *             lattice are not plain;
 *   distance  d(c) = the Chebyshev distance in cells from c to the nearest cell that is not plain, capped at
 *             threshold[n_level - 1];
 *   level     of a cell: the largest l < n_level such that the block of 2^l x 2^l cells that holds it, aligned at global
 *             cell indices (i0 + ci and j0 + cj rounded down to multiples of 2^l), lies wholly in the lattice and min d over
 *             it is at least threshold[l].  Such a block is a leaf.  threshold[0] = 0 and
 *             threshold[l] >= threshold[l - 1] + 2^(l - 1): leaves that share a side then differ by at most one level;
 *   faces     a level 0 cell emits what padne_polymesh_create emits for it.  Of a leaf of level l >= 1 the lower left cell
 *             emits for all, from the leaf's corners v00, v10, v11, v01: a side hangs when the cell across it has a lower
 *             level; no side hangs: (v00, v10, v11), (v00, v11, v01); otherwise, with c the lattice vertex at the centre and
 *             the ring v00, [mid S], v10, [mid E], v11, [mid N], v01, [mid W] (a midpoint on a hanging side only), the faces
 *             (c, ring[k], ring[k + 1]) cyclically from v00: 5 to 8, right-isosceles, counter-clockwise;
 *   numbers   as padne_polymesh_fetch states them; a leaf's faces stand at its lower left cell.
 * With n_level = 1 the result is padne_polymesh_create's bit for bit.  level_cells_out[n_poly][n_level] (may be NULL): the
 * cells of every polygon's lattice by level.  The handle is padne_polymesh_create's: _fetch, _arrays, _destroy.
 * PADNE_E_INVALID, beyond that entry's: n_level outside 1 .. 6, threshold[0] != 0, a threshold below the one before it plus
 * 2^(l - 1), a seed coordinate that is not finite, 2^24 seeds or more, n_seed > 0 with seed_xy NULL. */
int padne_polymesh_create_graded(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                                 const double *ring_xy, double h, double snap, int64_t n_level, const int32_t *threshold,
                                 int64_t n_seed, const double *seed_xy, int64_t *vertex_count_out, int64_t *face_count_out,
                                 int64_t *level_cells_out, padne_polymesh **out);
/* xy_out[sum of the vertex counts][2]; tri_out[sum of the face counts][3], counter-clockwise, with the vertex indices of
 * their own polygon's mesh; kind_out[sum of the vertex counts]: 0 a lattice vertex, 1 a lattice vertex snapped onto the
 * boundary, 2 a cut vertex on a lattice edge.  Polygon by polygon: lattice vertices row-major, then cuts by lattice vertex
 * and family (E, N, NE); faces in cell order, the lower triangle first. */
int padne_polymesh_fetch(padne_ctx *ctx, const padne_polymesh *pm, double *xy_out, int32_t *tri_out, int32_t *kind_out);
int padne_polymesh_arrays(const padne_polymesh *pm, const void **xy_dev, const void **tri_dev, const void **kind_dev);
int padne_polymesh_destroy(padne_polymesh *pm);     /* NULL is accepted */

/* ---- connectivity pre-pass: which polygons does a point touch ---------------------------------
 * Stands where the reference's STRtree query and shapely's intersects / contains stand (padne/solver.py:84-148, 263-330);
 * DESIGN.md, "Connectivity pre-pass"; the rule, expression by expression, at the top of csrc/connectivity.hip, restated in
 * tests/connectivity_ref.py.  One call locates n_query points in a batch of polygons laid out as padne_polymesh_create takes
 * them (rings without a closing duplicate, orientation free).  Polygon p belongs to group poly_group[p] >= 0 (its layer),
 * ascending over the batch; query q = query_xy[q][2] to query_group[q] >= 0 and meets the polygons of its own group only.
 *   segments  for every ring vertex i, from the previous vertex of the same ring (cyclic) (xj, yj) to (xi, yi);
 *   box       the exact least and greatest x and y of the polygon's ring vertices; a query outside the closed box has kind 0;
 *   crossing  (yi > py) != (yj > py) && px < (xj - xi) * (py - yi) / (yj - yi) + xi, rounded as written; inside when the
 *             crossings over all rings are odd (the even-odd rule of padne_thermal_set_sources and the grid mesher);
 *   boundary  on when for some segment (xi - xj) * (py - yj) - (yi - yj) * (px - xj) == 0 and min(xi, xj) <= px <= max(xi, xj)
 *             and min(yi, yj) <= py <= max(yi, yj).  Exact, no tolerance: it sees every ring vertex, every point of an
 *             axis-parallel segment and every point where the products are exact; a point computed onto a slanted segment is
 *             in general not seen as on it and counts by parity;
 *   kind      of (query, polygon): 2 when on, else 1 when inside, else 0; a hit is kind != 0 (intersects), kind 1 is contains.
 * The result stays on the device behind a handle (destroyed before its context); hit_count_out sizes the arrays of
 * padne_polygons_locate_fetch: hit_ptr_out[n_query + 1], hit_poly_out[hits], hit_kind_out[hits], the hits of a query in
 * ascending polygon number.  Two calls give the same bits.  n_poly = 0 or n_query = 0 is valid and gives no hit.
 * PADNE_E_INVALID: a ring with fewer than 3 vertices, a polygon without a ring, a coordinate or a query that is not finite,
 * polygon groups that are not ascending, a negative group, a null pointer.  PADNE_E_TOOLARGE: 2^31 or more segments or hits.
 * One GPU.  What is built on it -- the graph over the hits, the pruned board, the display meshes of dead copper (the same
 * mesher; the reference's RELAXED constrained triangulation has no counterpart) -- and what was measured (0.93 ms for this
 * call on 40 004 polygons and 8 002 queries; no kernel trace): DESIGN.md, "Connectivity pre-pass". */
typedef struct padne_polyhits padne_polyhits; /* device-resident hits of one batch of queries */
int padne_polygons_locate(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                          const double *ring_xy, const int32_t *poly_group, int64_t n_query, const double *query_xy,
                          const int32_t *query_group, int64_t *hit_count_out, padne_polyhits **out);
int padne_polygons_locate_fetch(padne_ctx *ctx, const padne_polyhits *ph, int32_t *hit_ptr_out, int32_t *hit_poly_out,
                                int32_t *hit_kind_out);
int padne_polygons_locate_destroy(padne_polyhits *ph);     /* NULL is accepted */

/* ---- field sampler: the solved fields at points and on rasters --------------------------------
 * No reference counterpart in the solver: the reference's viewer reads out the nearest vertex / nearest face centroid under
 * the cursor (ui.py:192-267).  A sampler keeps the meshes, the potentials and one uniform grid of bins per layer on the
 * device until it is destroyed (before its context).  Meshes as in padne_power_density, mesh_layer[m] in [0, n_layer) the
 * layer of mesh m, potential_host[n_vert] in the global vertex numbering.  bins_hint: the number of bins of every layer's
 * grid, 0 = chosen from the face count (one bin per two faces); a layer whose lists come to more than 16 entries per face
 * is rebuilt with half the bins per side.
 *
 * The owner of a query point q on a layer: side(i, k) = orient(P, Q, q) for the edge from its lower global vertex P to its
 * higher Q, negated where the face runs the edge from Q to P (orient as in padne_kkt_current_report).  A face contains q
 * when its three sides are all >= 0 or all <= 0 and not all zero; the owner is the containing face with the lowest global
 * index among the meshes of the layer.  The index never changes an answer.  Per query: face_out = the owner (global face
 * index; -1 outside the copper, and then the other three are NaN); v_out = ((o_a / s) V_a + (o_b / s) V_b) + (o_c / s) V_c
 * with o_a the side of the edge opposite corner a = tri[0] (o_b, o_c alike) and s = (o_a + o_b) + o_c; j_out[2] and p_out
 * = the owner's row of padne_kkt_current_report's J_out and its padne_power_density value, bit for bit. */
int padne_sampler_create(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                         int32_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                         const int32_t *mesh_layer, const double *conductance, int32_t n_layer, const double *potential_host,
                         int64_t bins_hint, padne_sampler **out);
int padne_sampler_destroy(padne_sampler *s);
/* n query points xy_host[n][2] on `layer` -> face_out[n], v_out[n], j_out[n][2], p_out[n].  PADNE_E_INVALID for a null
 * handle, a layer out of range, a point that is not finite and more than 2^26 points. */
int padne_sampler_points(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *xy_host, int32_t *face_out,
                         double *v_out, double *j_out, double *p_out);
/* The same at the pixel centres (x0 + (i + 0.5) dx, y0 + (j + 0.5) dy) of a raster, row j and column i at j * width + i;
 * the kernel forms the points itself, nothing is uploaded.  PADNE_E_INVALID also for a pixel size that is not finite and
 * positive, a width or height below 1 and more than 2^26 pixels. */
int padne_sampler_raster(padne_ctx *ctx, padne_sampler *s, int32_t layer, double x0, double y0, double dx, double dy,
                         int64_t width, int64_t height, int32_t *face_out, double *v_out, double *j_out, double *p_out);
/* counts_out[6] = bins along x and y, list entries and faces of `layer`, then the candidate faces tested and the queries of
 * the last query call (any layer); seconds_out[3] = host time of the upload and of the index build in create, device time
 * of the last query kernel. */
int padne_sampler_stats(const padne_sampler *s, int32_t layer, int64_t *counts_out, double *seconds_out);

/* ---- thermal images: a block of temperature fields at points and on rasters ----------------------
 * No reference counterpart ("Thermal images").  A sampler may hold, next to its potentials, a block of n_field
 * <= 256 vertex fields fields_host[n_field][n_vert] (field-major, the global vertex numbering of padne_sampler_create) and
 * the sheet conductance kappa[n_mesh] [W/K] of every mesh (NULL: no heat flux).  The handle owns its copy; a second call
 * replaces the block, n_field = 0 removes it.  The index and padne_sampler_points / _raster are not touched.
 *
 * A field query locates q ONCE, by the owner rule above, and reads every field f out at it.  With a = tri[0], b = tri[1],
 * c = tri[2] of the owner and s = (o_a + o_b) + o_c:
 *     t_out[f][i]      = ((o_a / s) T_f[a] + (o_b / s) T_f[b]) + (o_c / s) T_f[c]       (v_out's formula)
 *     q_out[f][i][2]   = -kappa_m grad T_f on the owner, the gradient of j_out with corners as (tri[2], tri[0], tri[1]) and
 *                        kappa_m of the owner's mesh [W per mesh unit of length]
 *     hot_out[i], hot_field_out[i] = the maximum over the fields and the field that attains it, sequentially: field 0
 *                        first, replaced by a later field only when it is strictly greater
 * face_out[i] = the owner or -1; outside the copper t_out, q_out and hot_out are NaN and hot_field_out is -1.  t_out and
 * q_out may each be NULL: that output is neither computed nor stored, and a call with both NULL moves 16 bytes per sample.
 * No floating-point atomics: two calls give the same bits.  PADNE_E_INVALID, with nothing written, for a null handle, a
 * sampler without fields, q_out without kappa, a layer out of range, a point that is not finite, more than 2^26 samples,
 * and more than 2^28 values n_field x n where t_out or q_out is wanted. */
int padne_sampler_set_fields(padne_ctx *ctx, padne_sampler *s, int32_t n_field, const double *fields_host, const double *kappa);
int padne_sampler_field_points(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *xy_host,
                               int32_t *face_out, double *t_out, double *q_out, double *hot_out, int32_t *hot_field_out);
/* The same at the pixel centres of padne_sampler_raster's raster, plus the hottest pixel of every slot -- the n_field fields,
 * then hot_out: top_out[n_field + 1] the largest value among the pixels that have an owner and top_pixel_out[n_field + 1]
 * its flat index j * width + i, the lowest index on a tie; -infinity and -1 where no pixel lies on copper.  The maximum is
 * exact, so the fold's order does not show: per workgroup of 256 pixels a (value, pixel) top, then one workgroup per slot
 * over those.  PADNE_E_INVALID also for what padne_sampler_raster refuses. */
int padne_sampler_field_raster(padne_ctx *ctx, padne_sampler *s, int32_t layer, double x0, double y0, double dx, double dy,
                               int64_t width, int64_t height, int32_t *face_out, double *t_out, double *q_out, double *hot_out,
                               int32_t *hot_field_out, double *top_out, int64_t *top_pixel_out);

/* ---- thermal: steady-state temperature rise of the copper from Joule heating --------------------
 * No reference counterpart ("Thermal").  Unknown: theta = T - T_ambient [K] at the first n_potential unknowns of
 * the assembled electrical system `L` (the vertices of its meshes, then the internal nodes); multiplier rows take no part.
 *     A theta = b,   A = K_kappa + diag(h_m(v) M_v) + links
 * K_kappa: the cotangent stiffness of padne_assemble_system over the mesh `L` keeps on the device, with kappa[m] [W/K], the
 * thermal sheet conductance of mesh m, in the place of its electrical conductance, positive sign.  M_v = the sum over the
 * faces incident to vertex v, in ascending global face number, of A_f / 3 (A_f = |cross| / 2 as padne_kkt_error_estimate
 * forms it).  film[m] > 0 [W / (K length^2)]: every loss of mesh m to ambient.  Link e is a thermal conductance link_g[e]
 * [W/K] between the unknowns link_a[e] and link_b[e], stamped like a resistor (0: no link, nothing stamped).  A's stored
 * diagonal at a vertex is the one rounded sum (-K_ii) + film M_v; every other entry is K's, negated.
 * b_v = the sum over the faces incident to v, ascending, of P_f / 3, P_f [W] the Joule power of face f, then the node-heat
 * triples added in list order.  K and the links annihilate constants: sum_v film M_v theta_v = sum_v b_v.
 * The handle borrows `L` (which must outlive it) and is destroyed before its context.  PADNE_E_INVALID for a kappa or film
 * that is not finite and positive, a link conductance that is negative or not finite, a terminal out of range, a system
 * without a mesh, and an unknown whose row has no diagonal (a vertex without a face of non-zero area, an internal node no
 * link of positive conductance reaches).  Nothing crosses PCIe but the O(n_mesh + n_link) lists. */
typedef struct padne_thermal padne_thermal;
int padne_thermal_create(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int32_t n_mesh, const double *kappa,
                         const double *film, int64_t n_link, const int64_t *link_a, const int64_t *link_b, const double *link_g,
                         padne_thermal **out);
int padne_thermal_destroy(padne_thermal *th);     /* NULL is accepted */
/* borrowed handle of A (n_potential x n_potential; do not destroy) */
int padne_thermal_matrix(const padne_thermal *th, const padne_csr **csr_out);
/* M_out[n_vert] = M_v */
int padne_thermal_lumped(padne_ctx *ctx, const padne_thermal *th, double *M_out);
/* Solve for n_cols (1 .. 4096) heat loads at once.  face_power_host[n_cols][n_tri]: P_f of every column.  Node heat:
 * n_heat triples (heat_node[e] in [0, n_potential), heat_col[e] in [0, n_cols), heat_val[e] [W], finite), added to b in list
 * order after the faces' part.  b is formed on the device, 8 columns per launch, by a gather through the vertex -> faces
 * lists (no floating-point atomics), and all columns go through padne_solve_spd_dev together (opts null: rtol 1e-12, the
 * multigrid preconditioner; bit 0 of opts.flags is ignored: theta starts from zero, a zero column comes back as exact
 * zeros).  theta_host[n_cols][n_potential] (may be null: theta stays on the device for padne_thermal_report).
 * PADNE_E_NOTCONVERGED still keeps and returns the iterate. */
int padne_thermal_solve(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host, int64_t n_heat,
                        const int64_t *heat_node, const int32_t *heat_col, const double *heat_val, const padne_solve_opts *opts,
                        double *theta_host, padne_solve_info *info);
/* The heat load alone, as padne_thermal_solve forms it from the same arguments: b_out[n_cols][n_potential].  Nothing is
 * solved, and the handle then holds no solve to report on. */
int padne_thermal_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host, int64_t n_heat,
                       const int64_t *heat_node, const int32_t *heat_col, const double *heat_val, double *b_out);
/* The same with the face powers of every column of the block the last padne_kkt_finish_block left on the device of `plan`
 * (a plan of the `L` the handle was made from), computed there: P_f = sigma sum_{edges (i,k) of f} w_ik (V_i - V_k)^2 with
 * the assembly's |cot|/2 weights, the term padne_kkt_current_cases sums into mesh_power_out.  The powers never visit the
 * host; with the same triples theta has the bits of padne_thermal_solve fed with padne_thermal_face_power's result.
 * Preconditions and errors as padne_kkt_power_density_block. */
int padne_thermal_solve_kkt(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols, int64_t n_heat,
                            const int64_t *heat_node, const int32_t *heat_col, const double *heat_val,
                            const padne_solve_opts *opts, double *theta_host, padne_solve_info *info);
/* out_host[n_cols][n_tri]: the face powers of the last solve, as the handle holds them */
int padne_thermal_face_power(padne_ctx *ctx, const padne_thermal *th, int32_t n_cols, double *out_host);
/* Report on the theta of the last solve (n_cols its columns; n_tri, n_vert, n_mesh the mesh's).  Per column c:
 * face_mean_out[n_cols][n_tri] = ((theta_1 + theta_2) + theta_3) / 3 with the corners in the order of
 * padne_csr_power_density (may be null); per mesh m, mesh_max_out[c][m] = the largest theta of its vertices and
 * mesh_vertex_out[c][m] that vertex (global index, the lowest on a tie; -infinity and -1 for a mesh without vertices),
 * mesh_heat_out[c][m] = the sum of P_f over its faces and mesh_loss_out[c][m] = the sum of (film M_v) theta_v over its
 * vertices.  env_out[n_vert] = max_c theta_c per vertex and env_case_out[n_vert] the lowest column that attains it, visited
 * from column 0 and replaced on strictly greater only (both may be null: no envelope).  Sums of 256 items go down each wave
 * by halving strides and join as (0 + 1) + (2 + 3), tiles are summed per mesh in a fixed order: two calls give the same bits. */
int padne_thermal_report(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_tri, int64_t n_vert, int32_t n_mesh,
                         double *face_mean_out, double *mesh_max_out, int64_t *mesh_vertex_out, double *mesh_heat_out,
                         double *mesh_loss_out, double *env_out, int32_t *env_case_out);

/* ---- stack: heat conduction between layers through the dielectric --------------------------------
 * No reference counterpart ("Stack").  padne_thermal_create with the layer mesh_layer[m] in [0, n_layer) of every
 * mesh and n_pair pairs of layers (pair_a[p] != pair_b[p], every unordered pair at most once) with an areal conductance
 * pair_g[p] >= 0 [W / (K length^2)] (0: no pair).  For both sides (s -> t) of a pair and every vertex v of a mesh of layer s:
 * f = the owner face of xy[v] among the meshes of layer t by the rule of padne_sampler_create (none: nothing), lambda_k =
 * o_k / ((o_a + o_b) + o_c) the sampler's weights of its corners, and for k = 0, 1, 2 a thermal conductance
 *     c_k = ((0.5 pair_g) M_v) lambda_k       (c_k == 0: nothing)
 * between v and corner k of f.  G = the sum of these links: G_ij = -(the sum of the links between i and j, at most one from
 * each side), G_ii = the sum along row i, in ascending j, of (-G_ij) from 0.0.  The handle's matrix becomes A' = A + G on
 * the union pattern (one rounded add where both are stored, the diagonal included), with ascending columns, before the
 * entry returns: padne_thermal_matrix, the solves, padne_coupled_* and padne_transient_* work on A'.  G annihilates
 * constants: the film loss still equals the heat put in.  M_v, film M_v and the load are those of padne_thermal_create, and
 * with n_pair = 0 so is the matrix, bit for bit.  Meshes the system does not keep take no part.  No floating-point atomics:
 * two calls give the same bits.  PADNE_E_INVALID in addition for a mesh layer or pair layer out of range, a pair that
 * names one layer twice, a repeated pair and a pair_g that is negative or not finite.  Nothing crosses PCIe but the
 * O(n_mesh + n_link + n_pair) lists. */
int padne_thermal_create_stacked(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int32_t n_mesh, const double *kappa,
                                 const double *film, int64_t n_link, const int64_t *link_a, const int64_t *link_b,
                                 const double *link_g, int32_t n_layer, const int32_t *mesh_layer, int32_t n_pair,
                                 const int32_t *pair_a, const int32_t *pair_b, const double *pair_g, padne_thermal **out);
/* After a solve of n_cols columns on a handle of padne_thermal_create_stacked: flow_out[n_cols][n_pair] = the heat [W] that
 * flows from layer pair_a[p] to layer pair_b[p], the sum over the vertices i of layer a and their stored partners j in layer
 * b, ascending, of (-G_ij)(theta_i - theta_j); area_out[n_pair] = (the same sum of (-G_ij)) / pair_g[p], the coupled area
 * (0 for pair_g = 0).  n_cols = 0: the areas alone, no solve needed.  Tiles of 256 vertices of one mesh in the fixed order of
 * padne_thermal_report, the meshes of layer a in ascending order: two calls give the same bits. */
int padne_thermal_stack_flows(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *flow_out, double *area_out);
/* Read-outs of the coupling (tests).  counts_out[4] = pairs, sides (two per pair with pair_g > 0, in pair order, a -> b
 * first), (side, vertex) slots, stored off-diagonals of G. */
int padne_thermal_stack_sizes(const padne_thermal *th, int64_t *counts_out);
/* The slots, side by side, within a side the vertices of the source layer in ascending global order: side_offset_out
 * [sides + 1] the first slot of every side, vertex_out[n_query] the vertex, owner_out[n_query] its owner face (global, -1:
 * none), weight_out[n_query][3] = lambda_k and cond_out[n_query][3] = c_k (0 without an owner). */
int padne_thermal_stack_links(padne_ctx *ctx, const padne_thermal *th, int64_t n_query, int64_t *side_offset_out,
                              int32_t *vertex_out, int32_t *owner_out, double *weight_out, double *cond_out);
/* G: its off-diagonals as CSR (indptr_out[n_potential + 1], indices_out[nnz] ascending, data_out[nnz]) and its diagonal
 * diag_out[n_potential] (0 for a row without partners). */
int padne_thermal_stack_matrix(padne_ctx *ctx, const padne_thermal *th, int64_t nnz, int32_t *indptr_out, int32_t *indices_out,
                               double *data_out, double *diag_out);

/* ---- heat sources: footprints of components that dissipate watts ----------------------------------
 * No reference counterpart ("Heat sources").  Source s is a layer source_layer[s] in [0, n_layer), a polygon of
 * 3 to 256 vertices poly_xy[poly_ptr[s] .. poly_ptr[s + 1]][2] (poly_ptr[0] = 0) and, per column of a load, a power [W].
 * With mesh_layer[m] in [0, n_layer) the layer of every mesh of the handle's system, padne_thermal_set_sources builds on the
 * device, once per handle:
 *   - the list of s: the faces of the meshes of its layer whose centroid ((x1 + x2) + x3) / 3 (corners in the order of
 *     padne_thermal_report's face mean) lies inside the polygon by the even-odd rule -- the edge from (xj, yj), the
 *     previous vertex, to (xi, yi) crosses when (yi > cy) != (yj > cy) and cx < (xj - xi) * (cy - yi) / (yj - yi) + xi --
 *     in ascending global face number; counts_out[s] their number;
 *   - for a source that covers no centroid (fallback_out[s] = 1, counts_out[s] = 1) the one face that owns the vertex mean
 *     of the polygon (coordinates summed in vertex order, divided by n) by the rule of padne_sampler_create; where no face
 *     does, fallback_out[s] = 2 and the call fails with PADNE_E_INVALID: the source lies on no copper the system keeps;
 *   - area_out[s] = A_s, the sum of the list's face areas in tiles of 256 (the workgroup order of padne_thermal_report;
 *     thread i mod 256 adds tile i to its partial sum, one more workgroup sum joins the partial sums);
 *   - the sources of every face, in ascending source number.
 * The handle owns them until it is destroyed; a second call replaces them and n_source = 0 removes them.  From then on every
 * load the handle forms (padne_thermal_load, the solves, padne_coupled_solve_kkt, padne_transient_loads*) adds, after the
 * face gather and the node-heat triples, b[c][v] += the sum from 0.0 over the faces f around v, ascending, and over the
 * sources s of f, ascending, of ((area_f / A_s) * power[c][s]) / 3 -- with the powers padne_thermal_source_power gave last,
 * power[n_cols][n_source], finite and >= 0.  A handle with sources and no powers, or powers for another number of columns
 * than the load has, forms no load: PADNE_E_INVALID.  The weights of a source sum to 1, so its load sums to its power and
 * the film loss still equals the heat put in; the face powers of padne_thermal_face_power and the heat of
 * padne_thermal_report do not contain it.  No floating-point atomics: two calls give the same bits.  PADNE_E_INVALID also
 * for a layer out of range, a null pointer, a poly_ptr that does not ascend by 3 to 256, more than 4096 sources, a
 * coordinate that is not finite and a handle of another context. */
int padne_thermal_set_sources(padne_ctx *ctx, padne_thermal *th, int32_t n_layer, int32_t n_mesh, const int32_t *mesh_layer,
                              int32_t n_source, const int32_t *source_layer, const int64_t *poly_ptr, const double *poly_xy,
                              int64_t *counts_out, int32_t *fallback_out, double *area_out);
int padne_thermal_source_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *power);
/* Read-out of the lists (tests): ptr_out[n_source + 1] and face_out[n_entries], n_entries the sum of counts_out. */
int padne_thermal_source_lists(padne_ctx *ctx, const padne_thermal *th, int32_t n_source, int64_t n_entries, int64_t *ptr_out,
                               int32_t *face_out);
/* After a solve of n_cols columns: temperature_out[n_cols][n_source] = T_s - ambient = the sum over the list of s, in the
 * order of A_s, of (area_f / A_s) * mean[c][f], mean the face mean of padne_thermal_report.  Two calls give the same bits. */
int padne_thermal_source_report(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *temperature_out);

/* ---- film curves: film coefficients that depend on the temperature rise, by Newton rounds ----------
 * No reference counterpart ("Film curves").  The film of mesh m becomes a table: knots knot_ptr[m] ..
 * knot_ptr[m + 1] (1 to 64 of them) with h = knot_film[i] at the rise knot_rise[i] [K above ambient], linear between the
 * knots, held constant below the first (knot_rise = 0) and above the last.  About an iterate theta, vertex v of mesh m uses
 * the segment i that contains theta_v (the largest i with rise_i <= theta_v), s its slope (h_{i+1} - h_i) / (t_{i+1} - t_i),
 * s = 0 in both clamped ranges, and
 *     h = h_i + s * (theta - t_i)     g = h + s * theta     d_v = g * M_v     c_v = ((s * theta) * theta) * M_v     hM_v = h * M_v
 * A round solves (A - diag(hM0) + diag(d)) theta' = b + c from theta: the stored diagonal of vertex v is the one rounded sum
 * D0_v + (d_v - hM0_v), D0 the diagonal and hM0 = film[m] M_v as the create call left them (stack coupling included).  + - *
 * only on the device, -ffp-contract=off, fixed-order folds, no floating-point atomics: a host restatement reproduces every
 * bit, two calls give the same bits.  At theta = 0, and for a table of one knot, d_v = hM0_v in bits and c_v = 0.
 *
 * padne_thermal_set_film_curves follows padne_thermal_create or padne_thermal_create_stacked: the tables go to the device,
 * the place of every vertex row's diagonal is recorded, D0 and hM0 are copied.  PADNE_E_INVALID, with nothing changed, for a
 * table without knots or of more than 64, a rise that does not start at 0 and ascend strictly, a value that is not finite, a
 * film that is not positive, a loss density q(theta) = h(theta) theta that does not increase strictly (q' = h_i + s_i (2 theta
 * - t_i) must be positive at both ends of every segment; the message names the segment), an n_mesh that is not the handle's,
 * and a first knot_film of a mesh that differs in bits from the film[m] of the create call.  n_mesh = 0 removes the curves and
 * puts D0 and hM0 back.  A second call replaces the curves. */
int padne_thermal_set_film_curves(padne_ctx *ctx, padne_thermal *th, int32_t n_mesh, const int32_t *knot_ptr,
                                  const double *knot_rise, const double *knot_film);
/* The terms for any theta_host[n_vert] (tests): g_out, c_out and hM_out[n_vert], and *beyond_out = the number of vertices
 * above the last knot of a table of more than one knot.  A pure function of theta: no state of the handle changes. */
int padne_thermal_film_terms(padne_ctx *ctx, padne_thermal *th, const double *theta_host, double *g_out, double *c_out,
                             double *hM_out, int64_t *beyond_out);
/* Linearise about the held theta of a one-column solve (from_held = 1) or about zero (from_held = 0): the stored diagonals
 * are written through the recorded places, c and a copy of the iterate are kept for the next solve, and what was derived
 * from A's values (the multigrid hierarchy) is dropped and rebuilt by that solve. */
int padne_thermal_film_linearise(padne_ctx *ctx, padne_thermal *th, int32_t from_held);
/* On a handle with curves padne_thermal_solve, padne_thermal_solve_kkt and padne_coupled_solve_kkt take one column only
 * (PADNE_E_INVALID otherwise, nothing changed), add the kept c to the load behind the faces, the triples and the heat
 * sources, and start the iteration from the iterate of the last linearise (about zero: from zero, the bits of the solve
 * without curves).  padne_transient_create and padne_tsens_create refuse such a handle: PADNE_E_INVALID.
 * padne_thermal_solve_kkt_column: padne_thermal_solve_kkt for column `col` of the finished block of n_cols columns -- the
 * face powers of that one column go into the handle, then a one-column solve (the triples' columns are 0); also without
 * curves.  padne_thermal_resolve: the solve again on the load the last solve of the handle formed, plus the c of the last
 * linearise; nothing else is recomputed.  PADNE_E_INVALID without curves or without such a load. */
int padne_thermal_solve_kkt_column(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols, int32_t col,
                                   int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col, const double *heat_val,
                                   const padne_solve_opts *opts, double *theta_host, padne_solve_info *info);
int padne_thermal_resolve(padne_ctx *ctx, padne_thermal *th, const padne_solve_opts *opts, double *theta_host,
                          padne_solve_info *info);
/* After a one-column solve: *increment_out = max_v |theta_v - the iterate of the last linearise| over the vertices,
 * *vertex_out that vertex (the lowest on a tie; 0 and -1 without vertices), *beyond_out as padne_thermal_film_terms counts
 * it on the new theta; and hM_v = h(theta_v) M_v, so that padne_thermal_report's film loss is sum_v M_v q(theta_v). */
int padne_thermal_film_increment(padne_ctx *ctx, padne_thermal *th, double *increment_out, int64_t *vertex_out,
                                 int64_t *beyond_out);

/* ---- temperature sensitivities: what cools a hotspot, by adjoints ---------------------------------
 * No reference counterpart ("Temperature sensitivities").  After padne_kkt_finish_block of the n_cases load cases
 * (M x_c = r_c) and padne_thermal_solve_kkt of as many columns (A theta_c = b(x_c)) on `th`, an objective j of case c is the
 * temperature T_j = ambient + g_j^T theta_c.  With the corners (1, 2, 3) of a face as padne_thermal_report visits them and
 * w_ik the assembly's |cot| / 2 weights:
 *     A lambda_j = g_j;     lbar_f = ((lambda_1 + lambda_2) + lambda_3) / 3
 *     c_j = grad_x (sum_f lbar_f P_f(x) [+ sum_R ((lambda_a + lambda_b) / 2) (x_a - x_b)^2 / R]);     M^T mu_j = c_j
 *     e_f = lbar_f P_f + sigma sum_edges w_ik (mu_i - mu_k)(x_i - x_k)               (= sigma dT_j / dsigma_f)
 *     k_f = -kappa sum_edges w_ik (lambda_i - lambda_k)(theta_i - theta_k)           (= kappa dT_j / dkappa_f)
 * The handle borrows `th` and `plan` (both must outlive it) and owns device copies of what the later solves overwrite: the
 * cases' potentials and theta, field-major [n_cases][n_potential], then lambda [n_obj][n_potential] and the block c
 * [N][n_obj].  kappa[n_mesh]: the thermal sheet conductance the handle `th` was made with.  No floating-point atomics: two
 * calls give the same bits.  PADNE_E_INVALID for a null or foreign handle, a plan without a finished block of n_cases
 * columns or of another system, a thermal handle without a solve of n_cases columns, and a wrong n_mesh. */
typedef struct padne_tsens padne_tsens;
int padne_tsens_create(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cases, int32_t n_mesh, const double *kappa,
                       padne_tsens **out);
int padne_tsens_destroy(padne_tsens *ts);     /* NULL is accepted */
/* lambda_j for n_obj (1 .. 4096) objectives, formed and solved on the device: g never crosses PCIe.  Objective j reads case
 * obj_case[j].  obj_kind[j] = 0: the point obj_xy[j] on layer obj_arg[j] (mesh_layer[n_mesh]: the layer of every mesh) --
 * the owner face is the containing face of the layer with the lowest global number, by the sides of the field sampler, and
 * g_j is the sampler's weights o_k / s, s = (o_a + o_b) + o_c, at its corners; obj_unknown[3 j ..] and obj_weight[3 j ..]
 * RETURN the corners and weights.  Kind 1: g_j = the up to three pairs (obj_unknown[3 j + k], obj_weight[3 j + k]) the caller
 * lists (unknown -1: no pair).  Kind 2: heat source obj_arg[j] of the handle, g_v = the sum over the faces f of v's list,
 * front to back, that the source loads of (area_f / A_s) / 3: its load with unit power, so g_j^T theta is its footprint
 * temperature.  All columns go through one padne_solve_spd_dev on A, whose hierarchy exists from the forward solve (opts null:
 * the defaults of padne_thermal_solve).  probe_out[n_obj][n_probe] = lambda_j at the unknowns probe_idx.  PADNE_E_INVALID for
 * counts, cases, kinds, unknowns or sources out of range, values that are not finite, and a point on no face of its layer:
 * the message names the lowest such objective and nothing is solved.  PADNE_E_NOTCONVERGED keeps the iterate. */
int padne_tsens_thermal_adjoints(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, const int32_t *obj_case, const int32_t *obj_kind,
                                 const int32_t *obj_arg, const double *obj_xy, int64_t *obj_unknown, double *obj_weight,
                                 int32_t n_mesh, const int32_t *mesh_layer, int64_t n_probe, const int64_t *probe_idx,
                                 double *probe_out, const padne_solve_opts *opts, padne_solve_info *info);
/* The block c[N][n_obj] (row-major, the layout of the plan's right-hand sides) on the device, *r_dev_out, for
 * padne_kkt_solve_block_dev: row i of a vertex = the sum over the faces f of its list, front to back, of (2 lbar_f) * (sigma *
 * d), d the two edge terms w_ik (x_i - x_k) of f at i; then per resistor (res_a, res_b, res_R) in list order, grouped by the
 * unknown, +t at a and -t at b with t = (2 ((lambda_a + lambda_b) / 2)) * ((x_a - x_b) / R) (n_res = 0: no element heat); zero
 * on every other row.  One thread per unknown, the objectives in register chunks of 4.  PADNE_E_INVALID unless it follows
 * padne_tsens_thermal_adjoints of n_obj objectives, and for a terminal out of range or a resistance of 0. */
int padne_tsens_electrical_rhs(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int64_t n_res, const int64_t *res_a,
                               const int64_t *res_b, const double *res_R, const void **r_dev_out);
/* After padne_kkt_solve_block_dev of that block and padne_kkt_finish_block of n_obj columns on the handle's plan (mu is read
 * from the finished block): electrical_out, thermal_out, copper_out[n_obj][n_tri] = e_f / area_f, k_f / area_f and (e_f +
 * k_f) / area_f, and mesh_electrical_out, mesh_thermal_out[n_obj][n_mesh] the sums of e_f and k_f per mesh: tiles of 256
 * faces of one mesh, folded in the fixed order of padne_thermal_report.  PADNE_E_INVALID without that finished block. */
int padne_tsens_faces(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int64_t n_tri, int32_t n_mesh, double *electrical_out,
                      double *thermal_out, double *copper_out, double *mesh_electrical_out, double *mesh_thermal_out);
/* mesh_film_out[n_obj][n_mesh] = the sum over the vertices v of the mesh of -((film M_v lambda_v) theta_v) = film dT_j / dfilm
 * of the mesh, in tiles of 256 vertices and the fold of padne_thermal_report. */
int padne_tsens_vertices(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_mesh, double *mesh_film_out);
/* pair_out[n_obj][n_pair] = pair_g dT_j / dpair_g = -(the sum over the vertices i of layer a and their stored partners k in
 * layer b, ascending, of (-G_ik) ((lambda_i - lambda_k) (theta_i - theta_k))), in the order of padne_thermal_stack_flows.
 * n_pair: the pairs of the thermal handle (0 without a stack: nothing is written). */
int padne_tsens_pairs(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_pair, double *pair_out);
/* source_out[n_obj][n_source] = dT_j / dP_s [K/W] = padne_thermal_source_report's sum with lambda_j in the place of theta.
 * n_source: the heat sources of the thermal handle (0: nothing is written). */
int padne_tsens_sources(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_source, double *source_out);

/* ---- electro-thermal coupling: the copper's conductance follows its temperature ----------------
 * No reference counterpart ("Electro-thermal").  Face t of mesh m conducts sigma[m] * s[t],
 *     s[t] = 1 / (1 + alpha[m] * ((mean[t] + ambient) - conductance_temperature)),
 * mean[t] = ((theta_1 + theta_2) + theta_3) / 3 the face mean of padne_thermal_report.  The handle borrows the assembled
 * system `L`, whose values it rewrites in place, and the thermal handle `th` made from it (both must outlive it); it owns a
 * copy L0 of L's values, the scale of the next revalue, the scale of the last one and the face means of the last update.
 * Created with the copper at ambient: theta = 0, s = s^(0).  PADNE_E_INVALID for a null or foreign handle, an n_mesh that
 * is not the mesh's, a system whose rows' columns do not ascend (an uploaded matrix), an alpha or temperature that is not
 * finite, and a face whose 1 + alpha (T - T0) is not finite and positive (the message names the lowest such face).
 * Lumped resistors keep their resistance unless padne_coupled_set_resistors names them. */
typedef struct padne_coupled padne_coupled;
int padne_coupled_create(padne_ctx *ctx, padne_csr *L, padne_thermal *th, int32_t n_mesh, const double *alpha, double ambient,
                         double conductance_temperature, padne_coupled **out);
/* L gets the values it was assembled with again (NULL is accepted).  Destroy before `th`, `L` and the context. */
int padne_coupled_destroy(padne_coupled *cp);
/* back to the copper at ambient: the face means 0, the next scale s^(0) */
int padne_coupled_reset(padne_ctx *ctx, padne_coupled *cp);
/* the next revalue's scale from scale_host[n_tri] (finite and positive), for tests */
int padne_coupled_set_scale(padne_ctx *ctx, padne_coupled *cp, int64_t n_tri, const double *scale_host);
/* scale_out[n_tri]: the next revalue's scale (used = 0) or the last one's (used = 1); face_mean_out[n_tri] (may be null): the
 * face means of the last update */
int padne_coupled_get_scale(padne_ctx *ctx, const padne_coupled *cp, int32_t used, int64_t n_tri, double *scale_out,
                            double *face_mean_out);
/* L's values from L0 and the scale: L = L0 + sum_f (s_f - 1) sigma_m K_f.  Row v of a vertex: for every face f incident to
 * v in ascending global face number, with t_f = (s_f - 1) * sigma_m and the |cot|/2 weights of the face's two edges at v,
 * (v, a) then (v, b) in the face's cyclic corner order after v: c_a = t_f * w_a, c_b = t_f * w_b, acc[v, a] += c_a,
 * acc[v, b] += c_b, acc[v, v] = (acc[v, v] - c_a) - c_b, every acc starting at 0.0; then L[v, j] = L0[v, j] + acc[v, j].
 * Other rows are L0's.  The stiffness block stays symmetric bit for bit, and a scale of 1 everywhere gives the bits of L0.
 * What L had derived from its values (1 / diagonal, single-precision copy, multigrid hierarchy) is dropped; a padne_kkt plan
 * made from L before the call holds the old values and must not be used again.  The scale becomes the one "used". */
int padne_coupled_revalue(padne_ctx *ctx, padne_coupled *cp);
/* The next scale and *increment_out = max_t |mean[t] - previous mean[t]| from the theta of the thermal handle's last solve
 * (one column; theta_host null), or from theta_host[n_theta], n_theta = n_potential.  The maximum is taken per 256 faces
 * and then by one workgroup: two calls give the same bits. */
int padne_coupled_update(padne_ctx *ctx, padne_coupled *cp, int64_t n_theta, const double *theta_host, double *increment_out);
/* padne_thermal_solve_kkt for the one column of `plan`'s finished block with sigma[m] * s[t], s the used scale, in the
 * place of sigma[m] in the face powers (one product, then face_edge_power as before).  Arguments and errors as there. */
int padne_coupled_solve_kkt(padne_ctx *ctx, padne_coupled *cp, padne_kkt *plan, int64_t n_heat, const int64_t *heat_node,
                            const int32_t *heat_col, const double *heat_val, const padne_solve_opts *opts, double *theta_host,
                            padne_solve_info *info);
/* out_host[n_tri] = padne_kkt_power_density_block's value of the one column of `plan`'s finished block, times the used
 * scale of the face (one product on the device) */
int padne_coupled_power_density(padne_ctx *ctx, padne_coupled *cp, padne_kkt *plan, double *out_host);
/* Lumped resistors whose resistance follows their temperature ("Resistor coupling"): host arrays [n_res] of the
 * ends a, b (potential unknowns, vertices or internal nodes), the resistance R the system was assembled with, alpha and T0.
 * Resistor r conducts g_r s_r, g_r = 1 / R_r, with
 *     mean_r = (theta[a_r] + theta[b_r]) / 2,   s_r = 1 / (1 + alpha_r * ((mean_r + ambient) - t0_r)).
 * From then on padne_coupled_update, _update_transient and _reset also form s_r, the increment is the larger of the faces'
 * and the resistors' largest change of a mean (an invalid face is named first, then the lowest invalid resistor), and
 * padne_coupled_revalue follows the faces' pass, per row i a resistor touches and in ascending r, with t_r = (s_r - 1) * g_r,
 * by L[i, j] = L[i, j] + t_r and L[i, i] = L[i, i] - t_r as sequential rounded updates, j the other end; t_r == 0.0 writes
 * nothing and a resistor with a == b is left out.  The potential block stays symmetric bit for bit.  The resistors start at
 * ambient (mean 0).  n_res = 0 removes them: every entry then does, bit for bit, what it does on a handle that never had any.
 * PADNE_E_INVALID for an end outside [0, n_potential), an R that is not finite and positive, an alpha or T0 that is not
 * finite, a resistor whose 1 + alpha (ambient - T0) is not finite and positive, and a stamp without a stored entry in L; the
 * handle then keeps the resistors it had. */
int padne_coupled_set_resistors(padne_ctx *ctx, padne_coupled *cp, int64_t n_res, const int64_t *a, const int64_t *b,
                                const double *R, const double *alpha, const double *t0);
/* padne_coupled_get_scale for the resistors: scale_out[n_res] the next revalue's s_r (used = 0) or the last one's (used = 1);
 * mean_out[n_res] (may be null) the means of the last update.  n_res must be the number set. */
int padne_coupled_get_resistors(padne_ctx *ctx, const padne_coupled *cp, int32_t used, int64_t n_res, double *scale_out,
                                double *mean_out);

/* ---- transient: the copper's temperature rise under a schedule of load cases ---------------------
 * No reference counterpart ("Transient").  Backward Euler on C dtheta/dt + A theta = b(t), A the thermal handle's
 * operator and C = diag(c_m M_v) the lumped heat capacity of the vertices, capacity[m] = c_m [J / (K length^2)] the areal heat
 * capacity of mesh m; internal nodes carry none.  One step of length dt for column c running load case j = case_of_col[c]
 * (-1: sources off), every expression rounded as written:
 *     Cv[v] = c_m(v) * M_v;   cdt[v] = Cv[v] / dt
 *     S = A with S_vv = A_vv + cdt[v] for a vertex v (one rounded sum); every other entry has A's bits
 *     rhs[c][v] = cdt[v] * theta_n[c][v] + B[j][v] at a vertex (without the sum when j = -1); B[j][v], or 0.0, elsewhere
 *     S theta_{n+1}[c] = rhs[c]  by padne_solve_spd_dev with theta_n[c] as the initial guess
 * K and the links annihilate constants: sum_v Cv (theta_{n+1} - theta_n) / dt + sum_v film M_v theta_{n+1} = sum_v B[j]_v.
 * The handle borrows the thermal handle `th` (which must outlive it; destroy this one first) and owns Cv, S (A's pattern,
 * its own values, the dt they hold), the load table B[n_case][n_potential], the state theta[n_cols][n_potential], the
 * running envelope and the step counter.  The coupling is one-way: the face powers do not follow the temperature (with the
 * entries of "transient electro-thermal" below, which rewrite a load slot between two steps, they do).
 * PADNE_E_INVALID for a null or foreign handle, an n_mesh that is not the mesh's and a capacity that is not finite and
 * positive; a refused call leaves the handle as it was. */
typedef struct padne_transient padne_transient;
int padne_transient_create(padne_ctx *ctx, padne_thermal *th, int32_t n_mesh, const double *capacity, padne_transient **out);
int padne_transient_destroy(padne_transient *tr);     /* NULL is accepted */
/* Cv_out[n_vert] = Cv */
int padne_transient_capacity(padne_ctx *ctx, const padne_transient *tr, double *Cv_out);
/* The load table: B[j] = the heat load padne_thermal_load forms of column j of the same arguments, bit for bit (n_case
 * 1 .. 4096; the triples' columns name cases).  The face powers pass through the thermal handle's array: it then holds no
 * solve to report on.  A schedule under way ends: padne_transient_start follows. */
int padne_transient_loads(padne_ctx *ctx, padne_transient *tr, int32_t n_case, const double *face_power_host, int64_t n_heat,
                          const int64_t *heat_node, const int32_t *heat_col, const double *heat_val);
/* The same with the face powers of the block the last padne_kkt_finish_block left on the device of `plan`, as
 * padne_thermal_solve_kkt computes them: they never visit the host.  Preconditions and errors as there. */
int padne_transient_loads_kkt(padne_ctx *ctx, padne_transient *tr, padne_kkt *plan, int32_t n_case, int64_t n_heat,
                              const int64_t *heat_node, const int32_t *heat_col, const double *heat_val);
/* b_out[n_case][n_potential] = B, for tests */
int padne_transient_load_vectors(padne_ctx *ctx, const padne_transient *tr, int32_t n_case, double *b_out);
/* The state at time 0 for n_cols (1 .. 4096) columns: a column with initial_case[c] = -1 starts at ambient, exact zeros; one
 * with initial_case[c] = j from the steady state A theta = B[j], all such columns in one block solve on A from zero as
 * padne_thermal_solve does (opts and info as there).  The envelope becomes theta_0 with step 0, the step counter and the
 * time 0.  PADNE_E_INVALID before padne_transient_loads and for a case out of range.  PADNE_E_NOTCONVERGED keeps the iterate. */
int padne_transient_start(padne_ctx *ctx, padne_transient *tr, int32_t n_cols, const int32_t *initial_case,
                          const padne_solve_opts *opts, padne_solve_info *info);
/* S revalued for dt, as a borrowed handle (do not destroy), for tests */
int padne_transient_matrix(padne_transient *tr, double dt, const padne_csr **csr_out);
/* rhs_out[n_cols][n_potential]: the right-hand side the next step of length dt would solve; the state does not advance */
int padne_transient_rhs(padne_ctx *ctx, padne_transient *tr, double dt, const int32_t *case_of_col, double *rhs_out);
/* Advance every column by n_steps steps of length dt (finite and positive) under case_of_col[n_cols].  If the bits of dt
 * differ from the held ones S is revalued in place and what was derived from its values (1 / diagonal, single-precision
 * copies, multigrid hierarchy) is dropped; its x-window plan depends on the pattern only and stays.  Otherwise the hierarchy
 * built at the first step of a dt serves every later step -- the point of the design: step_setup_seconds_out is 0 on all
 * but that step.  opts null: rtol 1e-12, the multigrid preconditioner; bit 0 of opts.flags is forced on.  A step that ends
 * with PADNE_E_NOTCONVERGED keeps its iterate and the run goes on (the call then returns that code); info: the iterations
 * and seconds summed over the steps, the worst residuals.  Per-step results are written on the device and downloaded once
 * at the end: no host wait is added per step beyond the solver's own convergence polls.  Per step k, column c, mesh m:
 * mesh_max_out[k][c][m] and mesh_vertex_out[k][c][m] by the rule of padne_thermal_report (the lowest vertex on a tie,
 * -infinity and -1 for a mesh without vertices), mesh_stored_out = sum Cv theta [J] and mesh_loss_out = sum (film M_v) theta
 * [W] over the mesh's vertices, in the fixed order of padne_thermal_report's sums: two calls give the same bits.
 * probe_out[k][c][p] = theta[c][probe_idx[p]], exact bits (n_probe may be 0; an index may name an internal node).  After
 * every step the envelope takes, per column and vertex, a theta strictly greater than the held one together with the
 * global number of the step: the earliest step keeps a tie.  step_iterations_out[n_steps], step_residual_out[n_steps],
 * step_seconds_out[n_steps] (the iteration loop) and step_setup_seconds_out[n_steps]: of each step's solve (each may be null).  PADNE_E_INVALID before padne_transient_start,
 * for a dt that is not finite and positive, n_steps < 1, and a case or probe index out of range. */
int padne_transient_run(padne_ctx *ctx, padne_transient *tr, double dt, int32_t n_steps, const int32_t *case_of_col,
                        int32_t n_probe, const int64_t *probe_idx, const padne_solve_opts *opts, double *mesh_max_out,
                        int64_t *mesh_vertex_out, double *mesh_stored_out, double *mesh_loss_out, double *probe_out,
                        int32_t *step_iterations_out, double *step_residual_out, double *step_seconds_out,
                        double *step_setup_seconds_out, padne_solve_info *info);
/* the per-mesh results of padne_transient_run for the current state, [n_cols][n_mesh]; the envelope is left alone */
int padne_transient_report(padne_ctx *ctx, padne_transient *tr, double *mesh_max_out, int64_t *mesh_vertex_out,
                           double *mesh_stored_out, double *mesh_loss_out);
/* theta_out[n_cols][n_potential]: the current state */
int padne_transient_state(padne_ctx *ctx, const padne_transient *tr, double *theta_out);
/* env_out[n_cols][n_vert] and env_step_out[n_cols][n_vert]: the running envelope and the steps that attained it */
int padne_transient_envelope(padne_ctx *ctx, const padne_transient *tr, double *env_out, int32_t *env_step_out);
/* steps and time since the start, multigrid hierarchies built for S since creation (each may be null) */
int padne_transient_clock(const padne_transient *tr, int64_t *step_out, double *time_out, int64_t *hierarchies_out);

/* ---- adaptive transient: second-order steps with an error estimate ----------------------------------
 * No reference counterpart ("Adaptive transient").  Alexander's two-stage SDIRK2 on the transient handle, from
 * two backward-Euler solves on one matrix.  gamma = 1 - 1/sqrt(2) = 0.29289321881345247560 and q = (1 - gamma) / gamma =
 * sqrt(2) + 1 = 2.41421356237309504880, both as the nearest double.  One step of length dt from theta_n, for column c running
 * case j, every expression rounded as written:
 *     dts = gamma * dt
 *     stage 1:  S(dts) theta_1 = rhs(dts, theta_n, B[j])        exactly one step of padne_transient_run of length dts
 *     theta*[v] = theta_n[v] + q * (theta_1[v] - theta_n[v])   at a vertex; theta_1 at an internal node
 *     stage 2:  S(dts) theta_{n+1} = rhs(dts, theta*, B[j])     the same step with theta* in the place of theta_n
 *     est[v] = q * ((theta_1[v] - theta_n[v]) - (theta_{n+1}[v] - theta*[v]))   at a vertex
 *     err[c] = max_v |est[c][v]| [K]; an |est| that is not finite counts as +infinity
 * The caller decides what to do with err: padne_transient_accept, or another trial with another dt. */
/* The two stages into the handle's trial arrays; state, clock, envelope and load table are untouched.  err_out[n_cols] and
 * err_vertex_out[n_cols]: the estimate and the global vertex that attains it, the lowest on a tie (0.0 and -1 without
 * vertices), by the fixed order of padne_thermal_report's maxima per mesh and then over the meshes in ascending order,
 * replaced only on strictly greater: two calls give the same bits.  guess: what stage 2's solve starts from -- 0 theta_1,
 * 1 theta*, 2 theta_n + (theta_1 - theta_n) / gamma (internal nodes: theta_1); the result depends on it within the solve's
 * tolerance only.  Stage 1 starts from theta_n.  opts and info as in padne_transient_run, info summed over the stages;
 * stage_iterations_out[2] and stage_setup_seconds_out[2] (each may be null) per stage.  PADNE_E_NOTCONVERGED keeps the trial
 * and is reported.  PADNE_E_INVALID for what padne_transient_run refuses, a dt whose gamma * dt is not positive and a guess
 * out of range.  A live trial ends with the next padne_transient_try_step, padne_transient_start, padne_transient_run,
 * padne_transient_loads, padne_transient_loads_kkt and padne_transient_reserve_loads. */
int padne_transient_try_step(padne_ctx *ctx, padne_transient *tr, double dt, const int32_t *case_of_col, int32_t guess,
                             const padne_solve_opts *opts, double *err_out, int64_t *err_vertex_out,
                             int32_t *stage_iterations_out, double *stage_setup_seconds_out, padne_solve_info *info);
/* The live trial becomes the state (the arrays change places, nothing is copied): the step counter advances by one, the time
 * by the trial's dt, the envelope by the rule of padne_transient_run.  mesh_*_out[n_cols][n_mesh] and probe_out[n_cols][n_probe]
 * as one step of padne_transient_run writes them for theta_{n+1}; mesh_stage_loss_out[n_cols][n_mesh] the film loss of
 * theta_1 in the same fixed order.  With them (stored_{n+1} - stored_n) / dt + (1 - gamma) stage_loss + gamma loss_{n+1} =
 * the heat of the case, up to the solves' tolerance.  PADNE_E_INVALID without a live trial, and for a probe out of range. */
int padne_transient_accept(padne_ctx *ctx, padne_transient *tr, int32_t n_probe, const int64_t *probe_idx, double *mesh_max_out,
                           int64_t *mesh_vertex_out, double *mesh_stored_out, double *mesh_loss_out, double *mesh_stage_loss_out,
                           double *probe_out);
/* out[n_cols][n_potential] = theta_1 (which 0), theta* (1) or theta_{n+1} (2) of the live trial, for tests */
int padne_transient_trial(padne_ctx *ctx, const padne_transient *tr, int32_t which, double *out);

/* ---- transient electro-thermal: the resistivity follows the temperature over time ------------------
 * No reference counterpart ("Transient electro-thermal").  A coupling handle and a transient handle made on one
 * thermal handle, joined: a step from t_n while case j is on is padne_coupled_update_transient (the scale from theta_n),
 * padne_coupled_revalue, the caller's one-column electrical solve of case j on a fresh padne_kkt plan,
 * padne_coupled_transient_load (that solve's heat into slot j of the load table) and one step of padne_transient_run under
 * case j.  The nonlinear term is lagged by one step.  Every entry returns PADNE_E_INVALID, leaving the handles as they were,
 * for a null or foreign handle, handles that do not stand on one thermal handle, and what it names below. */
/* The load table as n_case (1 .. 4096) slots of exact zeros, for padne_coupled_transient_load to fill.  Like
 * padne_transient_loads, a schedule under way ends: padne_transient_start follows. */
int padne_transient_reserve_loads(padne_ctx *ctx, padne_transient *tr, int32_t n_case);
/* B[slot] = the heat load padne_coupled_solve_kkt forms before it solves, bit for bit: the face powers of the one column the
 * last padne_kkt_finish_block left on `plan` with sigma[m] * s[t], s the used scale, a third of each to every corner, the
 * node-heat triples (columns 0), the thermal handle's heat sources with the powers set for one column.  The state, the
 * clock, the envelope and a schedule under way are untouched: the next step under case `slot` uses the new load.  The same
 * launch sequence writes mesh_heat_out[n_mesh], the sum of every mesh's face powers [W] in the fixed order of
 * padne_thermal_report's sums: two calls give the same bits.  The face powers pass through the thermal handle's array, which
 * then holds no solve to report on.  PADNE_E_INVALID for a slot out of range (or no table), an n_mesh that is not the mesh's,
 * a plan without a finished one-column block of this system, and what padne_thermal_solve refuses of the triples. */
int padne_coupled_transient_load(padne_ctx *ctx, padne_coupled *cp, padne_transient *tr, padne_kkt *plan, int32_t slot,
                                 int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col, const double *heat_val,
                                 int32_t n_mesh, double *mesh_heat_out);
/* padne_coupled_update reading column `col` of the transient handle's state on the device: the bits of padne_coupled_update
 * given that theta from the host, and no vector crosses to the host.  PADNE_E_INVALID before padne_transient_start and for a
 * column out of range; for a face whose 1 + alpha (T - T0) is not finite and positive, the message of padne_coupled_update. */
int padne_coupled_update_transient(padne_ctx *ctx, padne_coupled *cp, const padne_transient *tr, int32_t col,
                                   double *increment_out);
/* *min_out, *max_out: the smallest and the largest used scale over the faces, per 256 faces and then by one workgroup (exact:
 * no rounding is involved).  PADNE_E_INVALID for a mesh without faces. */
int padne_coupled_scale_range(padne_ctx *ctx, const padne_coupled *cp, double *min_out, double *max_out);

/* ---- periodic steady state: the Krylov arithmetic of a duty cycle's period map ---------------------
 * No reference counterpart ("Periodic steady state").  The period map of padne_transient_run under a fixed
 * schedule is affine, theta(T) = Phi theta(0) + d, so the periodic state solves (I - Phi) theta* = d.  The caller runs GMRES
 * without restart on it, per column, all columns in lockstep; Phi v is one period of padne_transient_run from v with every
 * column's sources off.  These entries put a state into the transient handle and keep the basis on the device.
 * <x, y>_C = sum_v Cv[v] x[v] y[v] over the vertices, in which Phi is self-adjoint.  Vectors carry all n_potential entries;
 * dots, norms and maxima run over the vertices only.  Every expression rounded as written:
 *     dot      term[v] = (Cv[v] * w[v]) * v_i[v], up to 8 basis vectors per pass over w; per tile of 256 vertices of the
 *              column's whole vertex range in the fixed order of padne_thermal_report's sums, the tiles folded by one
 *              workgroup whose thread t takes tiles t, t + 256, ... front to back
 *     update   s = 0.0; s = s + d_i * v_i[e] for i ascending; w[e] = w[e] - s
 *     combine  a = base[e]; a = a + c_i * v_i[e] for i ascending
 *     top      the largest |a| over the vertices, the lowest vertex on a tie, by the same tiles and fold; a value that is not
 *              finite counts as +infinity; 0.0 and -1 without vertices
 * No floating-point atomics: two calls give the same bits.  The handle borrows a started transient handle `tr` (destroy this
 * one first) and owns x0, r0, w and the basis V[max_vectors][n_cols][n_potential] in the context's pool, n_cols that of the
 * start.  Every entry returns PADNE_E_INVALID, leaving both handles as they were, for a null or foreign handle, a transient
 * handle that has not been started or has been started anew with another number of columns, an index out of range and a
 * call out of the order stated below. */
typedef struct padne_periodic padne_periodic;
/* max_vectors 1 .. 4095.  PADNE_E_NOMEM when the basis does not fit. */
int padne_periodic_create(padne_ctx *ctx, padne_transient *tr, int32_t max_vectors, padne_periodic **out);
int padne_periodic_destroy(padne_periodic *pd);       /* NULL is accepted */
/* x0 = the state.  The basis and r0 hold nothing afterwards. */
int padne_periodic_mark(padne_ctx *ctx, padne_periodic *pd);
/* After padne_periodic_mark: r0 = state - x0; beta_out[c] = sqrt(<r0, r0>_C); max_out[c] = max_v |r0[c][v]| with
 * vertex_out[c]; v_0 = r0 / beta, exact zeros in a column whose beta is not positive (a frozen column).  The basis then
 * holds one vector. */
int padne_periodic_residual(padne_ctx *ctx, padne_periodic *pd, double *beta_out, double *max_out, int64_t *vertex_out);
/* state = v_j (a vector the basis holds).  The clock, the envelope and a live trial step are reset as by
 * padne_transient_start: step and time 0, the envelope the state with step 0.  The load table is untouched. */
int padne_periodic_load(padne_ctx *ctx, padne_periodic *pd, int32_t j);
/* j the newest vector of a basis that is not full: w = v_j - state, orthogonalised against v_0 .. v_j by classical
 * Gram-Schmidt applied twice (per pass the dots of w, then one update), h_out[c][i] = the sum of the two passes'
 * coefficients for i <= j, h_out[c][j + 1] = sqrt(<w, w>_C) of the result, v_{j+1} = w / h_out[c][j + 1], exact zeros in a
 * column where that is not positive.  h_out[n_cols][j + 2].  The state is left alone. */
int padne_periodic_push(padne_ctx *ctx, padne_periodic *pd, int32_t j, double *h_out);
/* After padne_periodic_residual, n_coef <= the vectors held: max_out[c] = max_v |r0 - sum_i coef[c][i] v_i| with
 * vertex_out[c]; coef[n_cols][n_coef].  Nothing is written on the device but the result. */
int padne_periodic_predict(padne_ctx *ctx, padne_periodic *pd, int32_t n_coef, const double *coef, double *max_out,
                           int64_t *vertex_out);
/* After padne_periodic_mark, n_y <= the vectors held: state = x0 + sum_i y[c][i] v_i, y[n_cols][n_y] (n_y = 0: x0's bits),
 * then reset as in padne_periodic_load. */
int padne_periodic_combine(padne_ctx *ctx, padne_periodic *pd, int32_t n_y, const double *y);
/* out[n_cols][n_potential] = v_j; j = -1: r0, j = -2: x0.  For tests. */
int padne_periodic_vector(padne_ctx *ctx, const padne_periodic *pd, int32_t j, double *out);
/* v_j = in[n_cols][n_potential] for j up to the number of vectors held (the basis then holds j + 1 at the least); j = -1:
 * r0, j = -2: x0, both then count as formed; j = -3: the state, reset as in padne_periodic_load.  For tests: the kernels on
 * vectors of the caller. */
int padne_periodic_put(padne_ctx *ctx, padne_periodic *pd, int32_t j, const double *in);

/* ---- introspection for benchmarks ---------------------------------------------------------- */
/* algorithmic bytes of one CSR SpMV: 12*nnz + 20*n_rows + 4   */
int64_t padne_spmv_algorithmic_bytes(const padne_csr *m);
/* average device time (seconds) of `repeat` back-to-back SpMV launches measured with HIP
 * events on the context stream, after `warmup` untimed launches */
int padne_spmv_time(padne_ctx *ctx, const padne_csr *m, const void *x_dev, void *y_dev,
                    int warmup, int repeat, double *seconds_per_launch);

/* the same two for the 8-vector product: 12*nnz + 4*n_rows + 16*n_rows*8 + 4 bytes */
int64_t padne_spmm8_algorithmic_bytes(const padne_csr *m);
int padne_spmm8_time(padne_ctx *ctx, const padne_csr *m, const void *x_dev, void *y_dev,
                     int warmup, int repeat, double *seconds_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* PADNE_HIP_H */
