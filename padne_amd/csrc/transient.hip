// Transient temperature rise of the copper under a schedule of load cases ("Transient").  No reference counterpart.
//
// Backward Euler on  C dtheta/dt + A theta = b(t)  with the thermal handle's A = K_kappa + diag(h M_v) + links and the lumped
// heat capacity C = diag(c_m M_v) of the vertices (internal nodes carry none: their rows stay A's, they follow the copper
// algebraically).  One step of length dt for column c, which runs load case j = case_of_col[c] (-1: sources off):
//
//     Cv[v]     = c_m(v) * M_v                       one product, kept on the handle
//     cdt[v]    = Cv[v] / dt                         one division
//     S         = A, with S_vv = A_vv + cdt[v] for v < n_vert (one rounded sum); every other entry has A's bits
//     rhs[c][v] = cdt[v] * theta_n[c][v] + B[j][v]   v < n_vert: one product, one sum; without the sum when j = -1
//     rhs[c][v] = B[j][v], or 0.0 when j = -1        v >= n_vert
//     S theta_{n+1}[c] = rhs[c]                      padne_solve_spd_dev from theta_n (bit 0 of the flags)
//
// S has A's pattern, so one x-window plan serves every dt, and S is better conditioned than A; the multigrid hierarchy built
// at the first step of a dt is reused by every later step of that dt.  K and the links annihilate constants, so every step
// obeys  sum_v Cv (theta_{n+1} - theta_n) / dt + sum_v hM_v theta_{n+1} = sum_v B[j]_v  up to the solve's tolerance.
//
// Kernels in the idiom of thermal.hip: one thread per vertex and column, workgroups of 256, field-major [column][vertex]
// arrays, no floating-point atomics, the report's sums in the fixed order of error.hpp.  All of them are streams bound by
// memory: the right-hand side moves 24 bytes per vertex and column (+ 8 for Cv, shared between the columns through the
// cache), the report reads theta once (8 bytes, + 12 for the envelope, + 16 for hM and Cv shared between the columns).
// Compiled with -ffp-contract=off: the expressions round as written, a numpy restatement reproduces them.
#include "thermal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace padne {                            // (struct padne_transient: thermal.hpp)

// Cv[v] = c_m(v) * M_v
__global__ __launch_bounds__(256) void transient_capacity_kernel(const long long n_vert, const int n_mesh,
                                                                 const long long *__restrict__ voff,
                                                                 const double *__restrict__ capacity,
                                                                 const double *__restrict__ Mv, double *__restrict__ Cv) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    Cv[v] = capacity[find_segment(voff, n_mesh, v)] * Mv[v];
}

// S's values from A's: the stored diagonal of vertex i becomes the one rounded sum A_ii + Cv[i] / dt, every other entry is
// copied.  One thread per row
__global__ __launch_bounds__(256) void transient_form_kernel(const long long n_rows, const long long n_vert,
                                                             const int32_t *__restrict__ rowptr, const int32_t *__restrict__ cols,
                                                             const double *__restrict__ a_vals, const double *__restrict__ Cv,
                                                             const double dt, double *__restrict__ s_vals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    for (int e = rowptr[i], e1 = rowptr[i + 1]; e < e1; ++e) {
        double a = a_vals[e];
        if (cols[e] == i && i < n_vert) a = a + Cv[i] / dt;
        s_vals[e] = a;
    }
}

// rhs[c][i] of the step (the top of this file); c = blockIdx.y, case_of_col[n_cols] on the device.  mode 0: the step's
// right-hand side; mode 1: the steady load of a start, B[j] or 0.0 (theta is not read)
__global__ __launch_bounds__(256) void transient_rhs_kernel(const long long n_pot, const long long n_vert,
                                                            const int *__restrict__ case_of_col, const double *__restrict__ Cv,
                                                            const double dt, const double *__restrict__ theta,
                                                            const double *__restrict__ B, const int mode,
                                                            double *__restrict__ rhs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    const long long at = (long long)blockIdx.y * n_pot + i;
    const int j = case_of_col[blockIdx.y];
    double r;
    if (mode == 0 && i < n_vert) {
        r = (Cv[i] / dt) * theta[at];
        if (j >= 0) r = r + B[(long long)j * n_pot + i];
    } else {
        r = j >= 0 ? B[(long long)j * n_pot + i] : 0.0;
    }
    rhs[at] = r;
}

// The report pass of one step.  Per vertex of a tile (256 vertices of one mesh, the layout of thermal_report_vertex_kernel)
// and column c = blockIdx.y, theta[c][v] is read once: per tile the stored heat sum of Cv[v] theta and the film loss sum of
// hM[v] theta in the fixed order of error.hpp, and the largest theta with its vertex (the lowest on a tie).  The envelope in
// the same pass -- env_mode 1: env = theta, env_step = step (a start); env_mode 2: replaced where theta is strictly greater
// (the earliest step keeps a tie); env_mode 0: untouched
__global__ __launch_bounds__(256) void transient_report_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                               const long long *__restrict__ voff, const long long n_pot,
                                                               const long long n_vert, const long long n_blocks,
                                                               const double *__restrict__ theta, const double *__restrict__ hM,
                                                               const double *__restrict__ Cv, double *__restrict__ tile_stored,
                                                               double *__restrict__ tile_loss, double *__restrict__ tile_max,
                                                               long long *__restrict__ tile_vert, const int env_mode,
                                                               const int step, double *__restrict__ env,
                                                               int *__restrict__ env_step) {
    __shared__ double red_s[4], red_l[4], red_v[4];
    __shared__ long long red_f[4];
    const long long b = blockIdx.x;
    const long long c = blockIdx.y;
    const int m = find_segment(vtile_off, n_mesh, b);
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    const bool live = v < voff[m + 1];
    double stored = 0.0, loss = 0.0, a = -INFINITY;
    long long f = kErrNoFace;
    if (live) {
        const double th = theta[c * n_pot + v];
        stored = Cv[v] * th;
        loss = hM[v] * th;
        a = th;
        f = v;
        if (env_mode == 1 || (env_mode == 2 && th > env[c * n_vert + v])) {
            env[c * n_vert + v] = th;
            env_step[c * n_vert + v] = step;
        }
    }
    stored = error_wave_sum(stored);
    loss = error_wave_sum(loss);
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_s[threadIdx.x >> 6] = stored;
        red_l[threadIdx.x >> 6] = loss;
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        tile_stored[c * n_blocks + b] = error_sum4(red_s);
        tile_loss[c * n_blocks + b] = error_sum4(red_l);
        tile_max[c * n_blocks + b] = a;
        tile_vert[c * n_blocks + b] = f;
    }
}

// Per (mesh m = blockIdx.x, column c = blockIdx.y), over the mesh's tiles in the fixed order of thermal_fold_kernel: the two
// sums, the largest tile maximum and its vertex (the lowest on a tie; -infinity and -1 for a mesh without tiles) at [c][m]
__global__ __launch_bounds__(256) void transient_fold_kernel(const int n_mesh, const long long n_blocks,
                                                             const long long *__restrict__ tile_off,
                                                             const double *__restrict__ tile_stored,
                                                             const double *__restrict__ tile_loss, const double *__restrict__ tile_v,
                                                             const long long *__restrict__ tile_f, double *__restrict__ out_stored,
                                                             double *__restrict__ out_loss, double *__restrict__ out_v,
                                                             long long *__restrict__ out_f) {
    __shared__ double red_s[4], red_l[4], red_v[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    const long long at = (long long)blockIdx.y * n_blocks;
    double s = 0.0, l = 0.0, a = -INFINITY;
    long long f = kErrNoFace;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) {
        s += tile_stored[at + i];
        l += tile_loss[at + i];
        error_merge(a, f, tile_v[at + i], tile_f[at + i]);
    }
    s = error_wave_sum(s);
    l = error_wave_sum(l);
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_s[threadIdx.x >> 6] = s;
        red_l[threadIdx.x >> 6] = l;
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long to = (long long)blockIdx.y * n_mesh + m;
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        out_stored[to] = error_sum4(red_s);
        out_loss[to] = error_sum4(red_l);
        out_v[to] = a;
        out_f[to] = f == kErrNoFace ? -1 : f;
    }
}

// out[c][p] = theta[c][probe[p]]; one thread per (column, probe)
__global__ __launch_bounds__(256) void transient_probe_kernel(const long long n_pot, const int n_cols, const int n_probe,
                                                              const long long *__restrict__ probe, const double *__restrict__ theta,
                                                              double *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_cols * n_probe) return;
    const long long c = t / n_probe;
    out[t] = theta[c * n_pot + probe[t - c * n_probe]];
}

static void transient_free(padne_transient *tr) {
    if (tr == nullptr) return;
    padne_ctx *ctx = tr->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    if (tr->S != nullptr) padne_csr_destroy(tr->S);
    for (void *p : {(void *)tr->Cv, (void *)tr->B, (void *)tr->theta, (void *)tr->env, (void *)tr->env_step, (void *)tr->trial[0],
                    (void *)tr->trial[1], (void *)tr->trial[2]})
        if (p != nullptr) pool_free(ctx, p);
    delete tr;
}

int transient_require(const char *entry, padne_ctx *ctx, const padne_transient *tr) {
    PADNE_REQUIRE(ctx && tr, "null argument");
    PADNE_REQUIRE(tr->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    return PADNE_OK;
}

bool transient_good_dt(double dt) { return std::isfinite(dt) && dt > 0.0; }

// S holds dt: revalued in place when the bits of dt differ from the held ones, and what was derived from its values dropped
int transient_set_dt(padne_transient *tr, double dt) {
    if (tr->have_dt && std::memcmp(&tr->dt, &dt, sizeof(double)) == 0) return PADNE_OK;
    padne_ctx *ctx = tr->ctx;
    csr_invalidate_values(tr->S);
    tr->have_dt = false;
    if (tr->n_pot > 0) {
        const padne_csr *A = tr->th->A;
        hipLaunchKernelGGL(transient_form_kernel, dim3(nblk(tr->n_pot)), dim3(256), 0, ctx->stream, tr->n_pot, tr->n_vert,
                           (const int32_t *)tr->S->rowptr, (const int32_t *)tr->S->cols, (const double *)A->vals,
                           (const double *)tr->Cv, dt, tr->S->vals);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    tr->dt = dt;
    tr->have_dt = true;
    return PADNE_OK;
}

int transient_check_cases(const padne_transient *tr, const int32_t *case_of_col, int n_cols, std::vector<int> *out) {
    PADNE_REQUIRE(case_of_col != nullptr, "null argument");
    out->resize((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) {
        PADNE_REQUIRE(case_of_col[c] >= -1 && case_of_col[c] < tr->n_case, "load case out of range (-1: sources off)");
        (*out)[(size_t)c] = case_of_col[c];
    }
    return PADNE_OK;
}

padne_solve_opts transient_opts(const padne_solve_opts *opts) {
    padne_solve_opts o;
    if (opts != nullptr) {
        o = *opts;
    } else {
        o.rtol = 1e-12;
        o.atol = 0.0;
        o.max_iter = 0;
        o.precond = 1;
        o.check_every = 0;
        o.flags = 0;
    }
    return o;
}

// the device side of a report pass (TransientPass, thermal.hpp): tile tables and tile results, made once per call
int transient_pass_init(padne_transient *tr, Scratch &sc, TransientPass *ps) {
    padne_ctx *ctx = tr->ctx;
    const std::vector<long long> vtile = thermal_tiles(tr->th->voff);
    ps->n_vb = vtile[(size_t)tr->n_mesh];
    PADNE_REQUIRE(ps->n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const size_t nm = (size_t)tr->n_mesh, cells = (size_t)tr->n_cols * (size_t)(ps->n_vb > 0 ? ps->n_vb : 1);
    PADNE_TRY(sc.alloc(&ps->d_vtile, nm + 1));
    PADNE_TRY(sc.alloc(&ps->d_tstored, cells));
    PADNE_TRY(sc.alloc(&ps->d_tloss, cells));
    PADNE_TRY(sc.alloc(&ps->d_tmax, cells));
    PADNE_TRY(sc.alloc(&ps->d_tvert, cells));
    // (pageable host memory: the copy is staged before the call returns, so the table may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(ps->d_vtile, vtile.data(), sizeof(long long) * (nm + 1), hipMemcpyHostToDevice, ctx->stream));
    return PADNE_OK;
}

// the report kernel and its fold on `theta`: the per-mesh results at out_*[n_cols][n_mesh] on the device
int transient_pass(padne_transient *tr, const TransientPass &ps, const double *theta, int env_mode, long long step,
                   double *out_stored, double *out_loss, double *out_max, long long *out_vert) {
    padne_ctx *ctx = tr->ctx;
    hipStream_t s = ctx->stream;
    const ErrorMesh M = error_mesh_of(tr->th->L);
    if (ps.n_vb > 0) {
        hipLaunchKernelGGL(transient_report_kernel, dim3((unsigned)ps.n_vb, (unsigned)tr->n_cols), dim3(256), 0, s, tr->n_mesh,
                           (const long long *)ps.d_vtile, M.voff, tr->n_pot, tr->n_vert, ps.n_vb, theta,
                           (const double *)tr->th->hM, (const double *)tr->Cv, ps.d_tstored, ps.d_tloss, ps.d_tmax, ps.d_tvert,
                           env_mode, (int)step, tr->env, tr->env_step);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(transient_fold_kernel, dim3((unsigned)tr->n_mesh, (unsigned)tr->n_cols), dim3(256), 0, s, tr->n_mesh, ps.n_vb,
                       (const long long *)ps.d_vtile, (const double *)ps.d_tstored, (const double *)ps.d_tloss,
                       (const double *)ps.d_tmax, (const long long *)ps.d_tvert, out_stored, out_loss, out_max, out_vert);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

int transient_rhs(padne_transient *tr, const int *d_case, double dt, int mode, const double *theta, double *d_rhs) {
    if (tr->n_pot == 0) return PADNE_OK;
    hipLaunchKernelGGL(transient_rhs_kernel, dim3(nblk(tr->n_pot), (unsigned)tr->n_cols), dim3(256), 0, tr->ctx->stream, tr->n_pot,
                       tr->n_vert, d_case, (const double *)tr->Cv, dt, theta, (const double *)tr->B, mode, d_rhs);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

int transient_probe(padne_transient *tr, int n_probe, const long long *d_probe, const double *theta, double *d_out) {
    const long long pcells = (long long)tr->n_cols * n_probe;
    hipLaunchKernelGGL(transient_probe_kernel, dim3(nblk(pcells)), dim3(256), 0, tr->ctx->stream, tr->n_pot, tr->n_cols, n_probe,
                       d_probe, theta, d_out);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

// the per-column case table on the device (the copy is complete when this returns: the host vector may go)
int transient_upload_cases(padne_transient *tr, Scratch &sc, const std::vector<int> &cases, int **d_case) {
    PADNE_TRY(sc.alloc(d_case, cases.size()));
    PADNE_HIP_CHECK(hipMemcpyAsync(*d_case, cases.data(), sizeof(int) * cases.size(), hipMemcpyHostToDevice, tr->ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(tr->ctx->stream));
    return PADNE_OK;
}

static int transient_set_loads(padne_ctx *ctx, padne_transient *tr, int32_t n_case, int64_t n_heat, const int64_t *heat_node,
                               const int32_t *heat_col, const double *heat_val) {
    const size_t count = (size_t)n_case * (size_t)(tr->n_pot > 0 ? tr->n_pot : 1);
    if (tr->B != nullptr) pool_free(ctx, tr->B);
    tr->n_case = 0;
    tr->started = false;                     // a running schedule names cases of the old table
    tr->trial_live = false;
    tr->B = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (tr->B == nullptr) return PADNE_E_NOMEM;
    PADNE_TRY(thermal_form_load(ctx, tr->th, n_case, n_heat, heat_node, heat_col, heat_val, tr->B));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    tr->n_case = n_case;
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_transient_create(padne_ctx *ctx, padne_thermal *th, int32_t n_mesh, const double *capacity,
                                      padne_transient **out) {
    PADNE_REQUIRE(ctx && th && capacity && out, "null argument");
    PADNE_REQUIRE(th->ctx == ctx, "padne_transient_create: the thermal handle belongs to another context");
    PADNE_REQUIRE(n_mesh == th->n_mesh, "n_mesh must be that of the system's mesh");
    PADNE_REQUIRE(th->film == nullptr, "a thermal handle with film curves takes no transient handle: the steps read A and hM as constants");
    for (int m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(std::isfinite(capacity[m]) && capacity[m] > 0.0, "the areal heat capacity of every mesh must be finite and positive");
    PADNE_REQUIRE(th->A->nnz <= 0x7fffffffLL, "the thermal operator");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_transient *tr = new padne_transient;
    tr->ctx = ctx;
    tr->th = th;
    tr->n_pot = th->n_pot;
    tr->n_vert = th->n_vert;
    tr->n_mesh = n_mesh;
    struct Guard {
        padne_transient *tr;
        ~Guard() { transient_free(tr); }
    } guard{tr};
    const padne_csr *A = th->A;
    PADNE_TRY(csr_alloc(ctx, A->n_rows, A->n_cols, A->nnz, &tr->S));
    PADNE_HIP_CHECK(hipMemcpyAsync(tr->S->rowptr, A->rowptr, sizeof(int32_t) * (size_t)(A->n_rows + 1), hipMemcpyDeviceToDevice, s));
    if (A->nnz > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(tr->S->cols, A->cols, sizeof(int32_t) * (size_t)A->nnz, hipMemcpyDeviceToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(tr->S->vals, A->vals, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToDevice, s));
    }
    tr->Cv = (double *)pool_alloc(ctx, sizeof(double) * (size_t)(tr->n_vert > 0 ? tr->n_vert : 1));
    if (tr->Cv == nullptr) return PADNE_E_NOMEM;
    Scratch sc(ctx);
    double *d_cap = nullptr;
    PADNE_TRY(sc.alloc(&d_cap, (size_t)n_mesh));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_cap, capacity, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    if (tr->n_vert > 0) {
        hipLaunchKernelGGL(transient_capacity_kernel, dim3(nblk(tr->n_vert)), dim3(256), 0, s, tr->n_vert, n_mesh,
                           error_mesh_of(th->L).voff, (const double *)d_cap, (const double *)th->Mv, tr->Cv);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));           // (the copy has read `capacity`)
    guard.tr = nullptr;
    *out = tr;
    return PADNE_OK;
}

extern "C" int padne_transient_destroy(padne_transient *tr) {
    transient_free(tr);
    return PADNE_OK;
}

extern "C" int padne_transient_capacity(padne_ctx *ctx, const padne_transient *tr, double *Cv_out) {
    PADNE_TRY(transient_require("padne_transient_capacity", ctx, tr));
    if (tr->n_vert == 0) return PADNE_OK;
    PADNE_REQUIRE(Cv_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(Cv_out, tr->Cv, sizeof(double) * (size_t)tr->n_vert, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_transient_loads(padne_ctx *ctx, padne_transient *tr, int32_t n_case, const double *face_power_host,
                                     int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col, const double *heat_val) {
    PADNE_TRY(transient_require("padne_transient_loads", ctx, tr));
    PADNE_TRY(thermal_check_heat(tr->th, n_case, n_heat, heat_node, heat_col, heat_val));
    PADNE_TRY(thermal_upload_power(ctx, tr->th, n_case, face_power_host));
    return transient_set_loads(ctx, tr, n_case, n_heat, heat_node, heat_col, heat_val);
}

extern "C" int padne_transient_loads_kkt(padne_ctx *ctx, padne_transient *tr, padne_kkt *plan, int32_t n_case, int64_t n_heat,
                                         const int64_t *heat_node, const int32_t *heat_col, const double *heat_val) {
    PADNE_TRY(transient_require("padne_transient_loads_kkt", ctx, tr));
    const double *V = nullptr;
    PADNE_TRY(thermal_kkt_block("padne_transient_loads_kkt", ctx, tr->th, plan, n_case, &V));
    PADNE_TRY(thermal_check_heat(tr->th, n_case, n_heat, heat_node, heat_col, heat_val));
    PADNE_TRY(thermal_kkt_face_power(ctx, tr->th, n_case, V, nullptr));
    return transient_set_loads(ctx, tr, n_case, n_heat, heat_node, heat_col, heat_val);
}

extern "C" int padne_transient_load_vectors(padne_ctx *ctx, const padne_transient *tr, int32_t n_case, double *b_out) {
    PADNE_TRY(transient_require("padne_transient_load_vectors", ctx, tr));
    PADNE_REQUIRE(tr->n_case >= 1 && n_case == tr->n_case, "padne_transient_load_vectors follows padne_transient_loads of as many cases");
    if (tr->n_pot == 0) return PADNE_OK;
    PADNE_REQUIRE(b_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(b_out, tr->B, sizeof(double) * (size_t)n_case * (size_t)tr->n_pot, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_transient_start(padne_ctx *ctx, padne_transient *tr, int32_t n_cols, const int32_t *initial_case,
                                     const padne_solve_opts *opts, padne_solve_info *info) {
    PADNE_TRY(transient_require("padne_transient_start", ctx, tr));
    PADNE_REQUIRE(tr->n_case >= 1, "padne_transient_start follows padne_transient_loads");
    PADNE_REQUIRE(n_cols >= 1 && n_cols <= 4096, "between 1 and 4096 columns");
    std::vector<int> cases;
    PADNE_TRY(transient_check_cases(tr, initial_case, n_cols, &cases));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (info != nullptr) memset(info, 0, sizeof(*info));
    tr->started = false;
    tr->trial_live = false;
    if (n_cols != tr->n_cols || tr->theta == nullptr) {
        for (void *p : {(void *)tr->theta, (void *)tr->env, (void *)tr->env_step, (void *)tr->trial[0], (void *)tr->trial[1],
                        (void *)tr->trial[2]})
            if (p != nullptr) pool_free(ctx, p);
        tr->theta = tr->env = tr->trial[0] = tr->trial[1] = tr->trial[2] = nullptr;
        tr->env_step = nullptr;
        tr->n_cols = 0;
        const size_t np = (size_t)n_cols * (size_t)(tr->n_pot > 0 ? tr->n_pot : 1), nv = (size_t)n_cols * (size_t)(tr->n_vert > 0 ? tr->n_vert : 1);
        tr->theta = (double *)pool_alloc(ctx, sizeof(double) * np);
        tr->env = (double *)pool_alloc(ctx, sizeof(double) * nv);
        tr->env_step = (int *)pool_alloc(ctx, sizeof(int) * nv);
        if (!tr->theta || !tr->env || !tr->env_step) return PADNE_E_NOMEM;
        tr->n_cols = n_cols;
    }
    const size_t count = (size_t)n_cols * (size_t)tr->n_pot;
    if (count > 0) PADNE_HIP_CHECK(hipMemsetAsync(tr->theta, 0, sizeof(double) * count, s));
    int rc = PADNE_OK;
    bool any = false;
    for (int c : cases) any = any || c >= 0;
    Scratch sc(ctx);
    if (any && count > 0) {
        // the steady state A theta = B[j] of every column that starts from one, from zero as padne_thermal_solve does: a
        // column that starts at ambient is a zero column and comes back as exact zeros
        int *d_case = nullptr;
        double *d_b = nullptr;
        PADNE_TRY(transient_upload_cases(tr, sc, cases, &d_case));
        PADNE_TRY(sc.alloc(&d_b, count));
        PADNE_TRY(transient_rhs(tr, d_case, 1.0, 1, tr->theta, d_b));
        padne_solve_opts o = transient_opts(opts);
        o.flags &= ~1;
        rc = padne_solve_spd_dev(ctx, tr->th->A, d_b, tr->theta, n_cols, &o, info);
        if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
    }
    tr->step = 0;
    tr->time = 0.0;
    // the envelope is theta_0, attained at step 0
    TransientPass ps;
    double *d_res = nullptr;
    long long *d_vert = nullptr;
    const size_t cells = (size_t)n_cols * (size_t)tr->n_mesh;
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_res, 3 * cells));
    PADNE_TRY(sc.alloc(&d_vert, cells));
    PADNE_TRY(transient_pass(tr, ps, tr->theta, 1, tr->step, d_res, d_res + cells, d_res + 2 * cells, d_vert));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    tr->started = true;
    return rc;
}

extern "C" int padne_transient_matrix(padne_transient *tr, double dt, const padne_csr **csr_out) {
    PADNE_REQUIRE(tr && csr_out, "null argument");
    PADNE_REQUIRE(transient_good_dt(dt), "dt must be finite and positive");
    PADNE_HIP_CHECK(hipSetDevice(tr->ctx->device));
    PADNE_TRY(transient_set_dt(tr, dt));
    *csr_out = tr->S;
    return PADNE_OK;
}

extern "C" int padne_transient_rhs(padne_ctx *ctx, padne_transient *tr, double dt, const int32_t *case_of_col, double *rhs_out) {
    PADNE_TRY(transient_require("padne_transient_rhs", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_rhs follows padne_transient_start");
    PADNE_REQUIRE(transient_good_dt(dt), "dt must be finite and positive");
    std::vector<int> cases;
    PADNE_TRY(transient_check_cases(tr, case_of_col, tr->n_cols, &cases));
    if (tr->n_pot == 0) return PADNE_OK;
    PADNE_REQUIRE(rhs_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t count = (size_t)tr->n_cols * (size_t)tr->n_pot;
    Scratch sc(ctx);
    int *d_case = nullptr;
    double *d_rhs = nullptr;
    PADNE_TRY(transient_upload_cases(tr, sc, cases, &d_case));
    PADNE_TRY(sc.alloc(&d_rhs, count));
    PADNE_TRY(transient_rhs(tr, d_case, dt, 0, tr->theta, d_rhs));
    PADNE_HIP_CHECK(hipMemcpyAsync(rhs_out, d_rhs, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_transient_run(padne_ctx *ctx, padne_transient *tr, double dt, int32_t n_steps, const int32_t *case_of_col,
                                   int32_t n_probe, const int64_t *probe_idx, const padne_solve_opts *opts, double *mesh_max_out,
                                   int64_t *mesh_vertex_out, double *mesh_stored_out, double *mesh_loss_out, double *probe_out,
                                   int32_t *step_iterations_out, double *step_residual_out, double *step_seconds_out,
                                   double *step_setup_seconds_out, padne_solve_info *info) {
    PADNE_TRY(transient_require("padne_transient_run", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_run follows padne_transient_start");
    PADNE_REQUIRE(transient_good_dt(dt), "dt must be finite and positive");
    PADNE_REQUIRE(n_steps >= 1 && n_steps <= 1000000 && tr->step + n_steps <= 0x7fffffffLL, "number of steps");
    PADNE_REQUIRE(n_probe >= 0 && n_probe <= 1000000, "number of probes");
    PADNE_REQUIRE(n_probe == 0 || (probe_idx && probe_out), "null argument");
    PADNE_REQUIRE(mesh_max_out && mesh_vertex_out && mesh_stored_out && mesh_loss_out, "null argument");
    for (int p = 0; p < n_probe; ++p) PADNE_REQUIRE(probe_idx[p] >= 0 && probe_idx[p] < tr->n_pot, "probe unknown out of range");
    std::vector<int> cases;
    PADNE_TRY(transient_check_cases(tr, case_of_col, tr->n_cols, &cases));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    tr->trial_live = false;                             // a trial step (sdirk.hip) stood on the state that now advances
    const int n_cols = tr->n_cols;
    const size_t count = (size_t)n_cols * (size_t)tr->n_pot, cells = (size_t)n_cols * (size_t)tr->n_mesh,
                 pcells = (size_t)n_cols * (size_t)n_probe, ns = (size_t)n_steps;
    padne_solve_info total;
    memset(&total, 0, sizeof(total));
    total.n_rhs = n_cols;
    if (info != nullptr) *info = total;
    PADNE_TRY(transient_set_dt(tr, dt));
    padne_solve_opts o = transient_opts(opts);
    o.flags |= 1;                                       // theta_n is the initial guess of the step
    Scratch sc(ctx);
    TransientPass ps;
    int *d_case = nullptr;
    long long *d_probe = nullptr, *d_vert = nullptr;
    double *d_rhs = nullptr, *d_max = nullptr, *d_stored = nullptr, *d_loss = nullptr, *d_pout = nullptr;
    PADNE_TRY(transient_upload_cases(tr, sc, cases, &d_case));
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_rhs, count));
    PADNE_TRY(sc.alloc(&d_max, ns * cells));
    PADNE_TRY(sc.alloc(&d_stored, ns * cells));
    PADNE_TRY(sc.alloc(&d_loss, ns * cells));
    PADNE_TRY(sc.alloc(&d_vert, ns * cells));
    if (n_probe > 0) {
        PADNE_TRY(sc.alloc(&d_probe, (size_t)n_probe));
        PADNE_TRY(sc.alloc(&d_pout, ns * pcells));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_probe, probe_idx, sizeof(long long) * (size_t)n_probe, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
    }
    int worst = PADNE_OK;
    for (int32_t k = 0; k < n_steps; ++k) {
        padne_solve_info one;
        memset(&one, 0, sizeof(one));
        if (count > 0) {
            PADNE_TRY(transient_rhs(tr, d_case, dt, 0, tr->theta, d_rhs));
            const bool fresh = tr->S->amg == nullptr;
            const int rc = padne_solve_spd_dev(ctx, tr->S, d_rhs, tr->theta, n_cols, &o, &one);
            if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
            if (rc == PADNE_E_NOTCONVERGED) worst = rc;      // the iterate is kept and the run goes on
            if (fresh && tr->S->amg != nullptr) ++tr->hierarchies;
        }
        tr->step += 1;
        tr->time += dt;
        PADNE_TRY(transient_pass(tr, ps, tr->theta, 2, tr->step, d_stored + (size_t)k * cells, d_loss + (size_t)k * cells, d_max + (size_t)k * cells,
                                 d_vert + (size_t)k * cells));
        if (n_probe > 0 && count > 0) PADNE_TRY(transient_probe(tr, (int)n_probe, d_probe, tr->theta, d_pout + (size_t)k * pcells));
        total.iterations += one.iterations;
        total.restarts += one.restarts;
        if (one.rel_residual > total.rel_residual) total.rel_residual = one.rel_residual;
        if (one.abs_residual > total.abs_residual) total.abs_residual = one.abs_residual;
        total.solve_seconds += one.solve_seconds;
        total.precond_setup_seconds += one.precond_setup_seconds;
        total.operator_complexity = one.operator_complexity;
        total.levels = one.levels;
        total.precond_fallbacks += one.precond_fallbacks;
        if (step_iterations_out != nullptr) step_iterations_out[k] = one.iterations;
        if (step_residual_out != nullptr) step_residual_out[k] = one.rel_residual;
        if (step_seconds_out != nullptr) step_seconds_out[k] = one.solve_seconds;
        if (step_setup_seconds_out != nullptr) step_setup_seconds_out[k] = one.precond_setup_seconds;
    }
    total.status = worst;
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_max, sizeof(double) * ns * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_vertex_out, d_vert, sizeof(long long) * ns * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_stored_out, d_stored, sizeof(double) * ns * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_loss_out, d_loss, sizeof(double) * ns * cells, hipMemcpyDeviceToHost, s));
    if (n_probe > 0 && count > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(probe_out, d_pout, sizeof(double) * ns * pcells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (info != nullptr) *info = total;
    if (worst == PADNE_E_NOTCONVERGED) set_error("a step of the transient run did not reach the tolerance (worst rel. residual %.3e)", total.rel_residual);
    return worst;
}

extern "C" int padne_transient_report(padne_ctx *ctx, padne_transient *tr, double *mesh_max_out, int64_t *mesh_vertex_out,
                                      double *mesh_stored_out, double *mesh_loss_out) {
    PADNE_TRY(transient_require("padne_transient_report", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_report follows padne_transient_start");
    PADNE_REQUIRE(mesh_max_out && mesh_vertex_out && mesh_stored_out && mesh_loss_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t cells = (size_t)tr->n_cols * (size_t)tr->n_mesh;
    Scratch sc(ctx);
    TransientPass ps;
    double *d_res = nullptr;
    long long *d_vert = nullptr;
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_res, 3 * cells));
    PADNE_TRY(sc.alloc(&d_vert, cells));
    PADNE_TRY(transient_pass(tr, ps, tr->theta, 0, tr->step, d_res, d_res + cells, d_res + 2 * cells, d_vert));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_stored_out, d_res, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_loss_out, d_res + cells, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_res + 2 * cells, sizeof(double) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_vertex_out, d_vert, sizeof(long long) * cells, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_transient_state(padne_ctx *ctx, const padne_transient *tr, double *theta_out) {
    PADNE_TRY(transient_require("padne_transient_state", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_state follows padne_transient_start");
    if (tr->n_pot == 0) return PADNE_OK;
    PADNE_REQUIRE(theta_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(theta_out, tr->theta, sizeof(double) * (size_t)tr->n_cols * (size_t)tr->n_pot, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_transient_envelope(padne_ctx *ctx, const padne_transient *tr, double *env_out, int32_t *env_step_out) {
    PADNE_TRY(transient_require("padne_transient_envelope", ctx, tr));
    PADNE_REQUIRE(tr->started, "padne_transient_envelope follows padne_transient_start");
    if (tr->n_vert == 0) return PADNE_OK;
    PADNE_REQUIRE(env_out && env_step_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t nv = (size_t)tr->n_cols * (size_t)tr->n_vert;
    PADNE_HIP_CHECK(hipMemcpyAsync(env_out, tr->env, sizeof(double) * nv, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipMemcpyAsync(env_step_out, tr->env_step, sizeof(int32_t) * nv, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_transient_clock(const padne_transient *tr, int64_t *step_out, double *time_out, int64_t *hierarchies_out) {
    PADNE_REQUIRE(tr != nullptr, "null argument");
    if (step_out != nullptr) *step_out = tr->step;
    if (time_out != nullptr) *time_out = tr->time;
    if (hierarchies_out != nullptr) *hierarchies_out = tr->hierarchies;
    return PADNE_OK;
}
