// Error-controlled second-order steps of the transient handle ("Adaptive transient").  No reference counterpart.
//
// Alexander's two-stage SDIRK2 (L-stable, stiffly accurate) on  C dtheta/dt + A theta = b(t), built from the backward-Euler
// step of transient.hip.  gamma = 1 - 1/sqrt(2), q = (1 - gamma) / gamma = sqrt(2) + 1.  One step of length dt from theta_n for
// a column running case j, every expression rounded as written:
//
//     dts        = gamma * dt                                       one rounded product
//     stage 1:     S(dts) theta_1     = rhs(dts, theta_n, B[j])     a backward-Euler step of length dts, from theta_n
//     theta*[v]  = theta_n[v] + q * (theta_1[v] - theta_n[v])       at a vertex; theta_1 at an internal node (only a guess there)
//     stage 2:     S(dts) theta_{n+1} = rhs(dts, theta*, B[j])      a backward-Euler step of length dts, from theta*
//     est[v]     = q * ((theta_1[v] - theta_n[v]) - (theta_{n+1}[v] - theta*[v]))      at a vertex
//     err[c]     = max_v |est[c][v]|, with the lowest vertex on a tie; an |est| that is not finite counts as +infinity
//
// S and rhs are transient.hip's (transient_form_kernel, transient_rhs_kernel); both stages share one matrix, so one hierarchy
// serves a run of equal dt.  Nothing but theta is carried from step to step.  est is the difference to the embedded
// first-order solution and is proportional to dt^2.
//
// Two new kernels, both streams bound by memory.  sdirk_extrapolate_kernel: one thread per unknown and column, 16 bytes read
// and 8 written (24 per unknown and column).  sdirk_estimate_kernel: on the 256-vertex tiles of transient_report_kernel it
// reads theta_n, theta_1 and theta_{n+1} once (24 bytes per vertex and column) and forms theta* again with the expression of
// the extrapolation, which -ffp-contract=off keeps to the same bits; per tile the largest |est| and its vertex through
// error.hpp's fixed order, folded per mesh by sdirk_fold_kernel.  No floating-point atomics: two calls give the same bits.
#include "thermal.hpp"

#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

namespace padne {

constexpr double kSdirkGamma = 0.29289321881345247560;      // 1 - 1/sqrt(2)
constexpr double kSdirkQ = 2.41421356237309504880;          // sqrt(2) + 1 = (1 - gamma) / gamma

// out[c][i] = a[c][i] + f * (b[c][i] - a[c][i]) at a vertex, b[c][i] at an internal node; c = blockIdx.y.  f = q gives theta*
__global__ __launch_bounds__(256) void sdirk_extrapolate_kernel(const long long n_pot, const long long n_vert, const double f,
                                                                const double *__restrict__ a, const double *__restrict__ b,
                                                                double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    const long long at = (long long)blockIdx.y * n_pot + i;
    const double t1 = b[at];
    out[at] = i < n_vert ? a[at] + f * (t1 - a[at]) : t1;
}

// Per tile b = blockIdx.x (256 vertices of one mesh) and column c = blockIdx.y: the largest |est| and its vertex at
// [c][b] (-infinity and kErrNoFace for a tile without a live lane, which no mesh with vertices has)
__global__ __launch_bounds__(256) void sdirk_estimate_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                             const long long *__restrict__ voff, const long long n_pot,
                                                             const long long n_blocks, const double q,
                                                             const double *__restrict__ theta_n, const double *__restrict__ theta_1,
                                                             const double *__restrict__ theta_new, double *__restrict__ tile_max,
                                                             long long *__restrict__ tile_vert) {
    __shared__ double red_v[4];
    __shared__ long long red_f[4];
    const long long b = blockIdx.x;
    const long long c = blockIdx.y;
    const int m = find_segment(vtile_off, n_mesh, b);
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    double a = -INFINITY;
    long long f = kErrNoFace;
    if (v < voff[m + 1]) {
        const double tn = theta_n[c * n_pot + v];
        const double d = theta_1[c * n_pot + v] - tn;
        const double star = tn + q * d;
        const double est = q * (d - (theta_new[c * n_pot + v] - star));
        a = fabs(est);
        if (!(a <= 1.7976931348623157e308)) a = INFINITY;       // NaN as well: it must not lose every comparison
        f = v;
    }
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) error_merge(a, f, red_v[w], red_f[w]);
        tile_max[c * n_blocks + b] = a;
        tile_vert[c * n_blocks + b] = f;
    }
}

// Per (mesh m = blockIdx.x, column c = blockIdx.y), over the mesh's tiles in the order of transient_fold_kernel: the largest
// tile maximum and its vertex at [c][m] (-infinity and -1 for a mesh without vertices)
__global__ __launch_bounds__(256) void sdirk_fold_kernel(const int n_mesh, const long long n_blocks,
                                                         const long long *__restrict__ tile_off, const double *__restrict__ tile_v,
                                                         const long long *__restrict__ tile_f, double *__restrict__ out_v,
                                                         long long *__restrict__ out_f) {
    __shared__ double red_v[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    const long long at = (long long)blockIdx.y * n_blocks;
    double a = -INFINITY;
    long long f = kErrNoFace;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) error_merge(a, f, tile_v[at + i], tile_f[at + i]);
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long to = (long long)blockIdx.y * n_mesh + m;
        for (int w = 1; w < 4; ++w) error_merge(a, f, red_v[w], red_f[w]);
        out_v[to] = a;
        out_f[to] = f == kErrNoFace ? -1 : f;
    }
}

static int sdirk_extrapolate(padne_transient *tr, double f, const double *a, const double *b, double *out) {
    if (tr->n_pot == 0) return PADNE_OK;
    hipLaunchKernelGGL(sdirk_extrapolate_kernel, dim3(nblk(tr->n_pot), (unsigned)tr->n_cols), dim3(256), 0, tr->ctx->stream, tr->n_pot,
                       tr->n_vert, f, a, b, out);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

static void sdirk_add(padne_solve_info *total, const padne_solve_info &one) {
    total->iterations += one.iterations;
    total->restarts += one.restarts;
    if (one.rel_residual > total->rel_residual) total->rel_residual = one.rel_residual;
    if (one.abs_residual > total->abs_residual) total->abs_residual = one.abs_residual;
    total->solve_seconds += one.solve_seconds;
    total->precond_setup_seconds += one.precond_setup_seconds;
    total->operator_complexity = one.operator_complexity;
    total->levels = one.levels;
    total->precond_fallbacks += one.precond_fallbacks;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_transient_try_step(padne_ctx *ctx, padne_transient *tr, double dt, const int32_t *case_of_col, int32_t guess,
                                        const padne_solve_opts *opts, double *err_out, int64_t *err_vertex_out,
                                        int32_t *stage_iterations_out, double *stage_setup_seconds_out, padne_solve_info *info) {
    PADNE_TRY(transient_require("padne_transient_try_step", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_try_step follows padne_transient_start");
    PADNE_REQUIRE(transient_good_dt(dt), "dt must be finite and positive");
    const double dts = kSdirkGamma * dt;
    PADNE_REQUIRE(transient_good_dt(dts), "dt must be finite and positive");
    PADNE_REQUIRE(tr->step + 1 <= 0x7fffffffLL, "number of steps");
    PADNE_REQUIRE(guess >= 0 && guess <= 2, "the initial guess of stage 2: 0 theta_1, 1 theta*, 2 theta_n + (theta_1 - theta_n) / gamma");
    PADNE_REQUIRE(err_out && err_vertex_out, "null argument");
    std::vector<int> cases;
    PADNE_TRY(transient_check_cases(tr, case_of_col, tr->n_cols, &cases));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    tr->trial_live = false;
    const int n_cols = tr->n_cols;
    const size_t count = (size_t)n_cols * (size_t)tr->n_pot, cells = (size_t)n_cols * (size_t)tr->n_mesh;
    padne_solve_info total;
    memset(&total, 0, sizeof(total));
    total.n_rhs = n_cols;
    if (info != nullptr) *info = total;
    for (double *&p : tr->trial) {
        if (p != nullptr) continue;
        p = (double *)pool_alloc(ctx, sizeof(double) * (count > 0 ? count : 1));
        if (p == nullptr) return PADNE_E_NOMEM;
    }
    double *t1 = tr->trial[0], *star = tr->trial[1], *tnew = tr->trial[2];
    PADNE_TRY(transient_set_dt(tr, dts));
    padne_solve_opts o = transient_opts(opts);
    o.flags |= 1;                                       // each stage starts from a guess
    Scratch sc(ctx);
    TransientPass ps;
    int *d_case = nullptr;
    double *d_rhs = nullptr, *d_max = nullptr;
    long long *d_vert = nullptr;
    PADNE_TRY(transient_upload_cases(tr, sc, cases, &d_case));
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_rhs, count));
    PADNE_TRY(sc.alloc(&d_max, cells));
    PADNE_TRY(sc.alloc(&d_vert, cells));
    int worst = PADNE_OK;
    padne_solve_info stage[2];
    memset(stage, 0, sizeof(stage));
    if (count > 0) {
        // stage 1: the step of padne_transient_run of length dts, on a copy of the state
        PADNE_TRY(transient_rhs(tr, d_case, dts, 0, tr->theta, d_rhs));
        PADNE_HIP_CHECK(hipMemcpyAsync(t1, tr->theta, sizeof(double) * count, hipMemcpyDeviceToDevice, s));
        bool fresh = tr->S->amg == nullptr;
        int rc = padne_solve_spd_dev(ctx, tr->S, d_rhs, t1, n_cols, &o, &stage[0]);
        if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
        if (rc == PADNE_E_NOTCONVERGED) worst = rc;
        if (fresh && tr->S->amg != nullptr) ++tr->hierarchies;
        // stage 2: the same step from theta*
        PADNE_TRY(sdirk_extrapolate(tr, kSdirkQ, tr->theta, t1, star));
        PADNE_TRY(transient_rhs(tr, d_case, dts, 0, star, d_rhs));
        if (guess == 2) {
            PADNE_TRY(sdirk_extrapolate(tr, 1.0 / kSdirkGamma, tr->theta, t1, tnew));
        } else {
            PADNE_HIP_CHECK(hipMemcpyAsync(tnew, guess == 0 ? t1 : star, sizeof(double) * count, hipMemcpyDeviceToDevice, s));
        }
        fresh = tr->S->amg == nullptr;
        rc = padne_solve_spd_dev(ctx, tr->S, d_rhs, tnew, n_cols, &o, &stage[1]);
        if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
        if (rc == PADNE_E_NOTCONVERGED) worst = rc;
        if (fresh && tr->S->amg != nullptr) ++tr->hierarchies;
    }
    if (ps.n_vb > 0) {
        hipLaunchKernelGGL(sdirk_estimate_kernel, dim3((unsigned)ps.n_vb, (unsigned)n_cols), dim3(256), 0, s, tr->n_mesh,
                           (const long long *)ps.d_vtile, error_mesh_of(tr->th->L).voff, tr->n_pot, ps.n_vb, kSdirkQ,
                           (const double *)tr->theta, (const double *)t1, (const double *)tnew, ps.d_tmax, ps.d_tvert);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sdirk_fold_kernel, dim3((unsigned)tr->n_mesh, (unsigned)n_cols), dim3(256), 0, s, tr->n_mesh, ps.n_vb,
                       (const long long *)ps.d_vtile, (const double *)ps.d_tmax, (const long long *)ps.d_tvert, d_max, d_vert);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<double> h_max(cells);
    std::vector<long long> h_vert(cells);
    PADNE_HIP_CHECK(hipMemcpyAsync(h_max.data(), d_max, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(h_vert.data(), d_vert, sizeof(long long) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    // the meshes in ascending order, replaced only on strictly greater: the lowest vertex keeps a tie
    for (int c = 0; c < n_cols; ++c) {
        double e = 0.0;
        long long at = -1;
        for (int m = 0; m < tr->n_mesh; ++m) {
            const size_t i = (size_t)c * (size_t)tr->n_mesh + (size_t)m;
            if (h_vert[i] >= 0 && (at < 0 || h_max[i] > e)) {
                e = h_max[i];
                at = h_vert[i];
            }
        }
        err_out[c] = e;
        err_vertex_out[c] = at;
    }
    for (int k = 0; k < 2; ++k) {
        sdirk_add(&total, stage[k]);
        if (stage_iterations_out != nullptr) stage_iterations_out[k] = stage[k].iterations;
        if (stage_setup_seconds_out != nullptr) stage_setup_seconds_out[k] = stage[k].precond_setup_seconds;
    }
    total.status = worst;
    if (info != nullptr) *info = total;
    tr->trial_dt = dt;
    tr->trial_live = true;
    if (worst == PADNE_E_NOTCONVERGED) set_error("a stage of the trial step did not reach the tolerance (worst rel. residual %.3e)", total.rel_residual);
    return worst;
}

extern "C" int padne_transient_accept(padne_ctx *ctx, padne_transient *tr, int32_t n_probe, const int64_t *probe_idx,
                                      double *mesh_max_out, int64_t *mesh_vertex_out, double *mesh_stored_out, double *mesh_loss_out,
                                      double *mesh_stage_loss_out, double *probe_out) {
    PADNE_TRY(transient_require("padne_transient_accept", ctx, tr));
    PADNE_REQUIRE(tr->started && tr->trial_live, "padne_transient_accept follows padne_transient_try_step");
    PADNE_REQUIRE(n_probe >= 0 && n_probe <= 1000000, "number of probes");
    PADNE_REQUIRE(n_probe == 0 || (probe_idx && probe_out), "null argument");
    PADNE_REQUIRE(mesh_max_out && mesh_vertex_out && mesh_stored_out && mesh_loss_out && mesh_stage_loss_out, "null argument");
    for (int p = 0; p < n_probe; ++p) PADNE_REQUIRE(probe_idx[p] >= 0 && probe_idx[p] < tr->n_pot, "probe unknown out of range");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t count = (size_t)tr->n_cols * (size_t)tr->n_pot, cells = (size_t)tr->n_cols * (size_t)tr->n_mesh,
                 pcells = (size_t)tr->n_cols * (size_t)n_probe;
    Scratch sc(ctx);
    TransientPass ps;
    double *d_res = nullptr, *d_stage = nullptr, *d_pout = nullptr;
    long long *d_vert = nullptr, *d_svert = nullptr, *d_probe = nullptr;
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_res, 3 * cells));
    PADNE_TRY(sc.alloc(&d_stage, 3 * cells));
    PADNE_TRY(sc.alloc(&d_vert, cells));
    PADNE_TRY(sc.alloc(&d_svert, cells));
    if (n_probe > 0) {
        PADNE_TRY(sc.alloc(&d_probe, (size_t)n_probe));
        PADNE_TRY(sc.alloc(&d_pout, pcells));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_probe, probe_idx, sizeof(long long) * (size_t)n_probe, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
    }
    // the trial becomes the state: the old state's array is the next trial's theta_{n+1}
    std::swap(tr->theta, tr->trial[2]);
    tr->trial_live = false;
    tr->step += 1;
    tr->time += tr->trial_dt;
    PADNE_TRY(transient_pass(tr, ps, tr->theta, 2, tr->step, d_res, d_res + cells, d_res + 2 * cells, d_vert));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_stored_out, d_res, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_loss_out, d_res + cells, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_res + 2 * cells, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_vertex_out, d_vert, sizeof(long long) * cells, hipMemcpyDeviceToHost, s));
    // the film loss of theta_1, by the same kernels (the tile results of the first pass have been folded: stream order)
    PADNE_TRY(transient_pass(tr, ps, tr->trial[0], 0, tr->step, d_stage, d_stage + cells, d_stage + 2 * cells, d_svert));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_stage_loss_out, d_stage + cells, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    if (n_probe > 0 && count > 0) {
        PADNE_TRY(transient_probe(tr, (int)n_probe, d_probe, tr->theta, d_pout));
        PADNE_HIP_CHECK(hipMemcpyAsync(probe_out, d_pout, sizeof(double) * pcells, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_transient_trial(padne_ctx *ctx, const padne_transient *tr, int32_t which, double *out) {
    PADNE_TRY(transient_require("padne_transient_trial", ctx, tr));
    PADNE_REQUIRE(tr->started && tr->trial_live, "padne_transient_trial follows padne_transient_try_step");
    PADNE_REQUIRE(which >= 0 && which <= 2, "which: 0 theta_1, 1 theta*, 2 theta_{n+1}");
    if (tr->n_pot == 0) return PADNE_OK;
    PADNE_REQUIRE(out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(out, tr->trial[which], sizeof(double) * (size_t)tr->n_cols * (size_t)tr->n_pot, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}
