// Electro-thermal coupling: the copper's sheet conductance follows its temperature ("Electro-thermal").  No
// reference counterpart.
//
// Face t of mesh m conducts sigma[m] * s[t] with
//
//     s[t] = 1 / (1 + alpha[m] * ((mean[t] + ambient) - t0)),    mean[t] = ((theta_1 + theta_2) + theta_3) / 3
//
// on the corner order of error_corners (the face mean of padne_thermal_report).  The electrical system is revalued in place
// from a kept copy L0 of its assembled values, in the correction form L = L0 + sum_f (s_f - 1) sigma_m K_f, which leaves
// every lumped stamp, internal-node row and multiplier row alone without knowing them.  Row v of a vertex, exactly:
//
//     for every face f of v's list (ascending global face number), with (g1, g2, g3) its corners,
//         w12 = cot_half(p1, p2, p3), w23 = cot_half(p2, p3, p1), w31 = cot_half(p3, p1, p2)     (thermal_face_power_kernel's)
//         t_f = (s[f] - 1) * sigma[m]
//         (a, w_a, b, w_b) = (g2, w12, g3, w31) if v == g1, (g3, w23, g1, w12) if v == g2, (g1, w31, g2, w23) if v == g3
//         c_a = t_f * w_a;  c_b = t_f * w_b
//         acc[v, a] = acc[v, a] + c_a;  acc[v, b] = acc[v, b] + c_b;  acc[v, v] = (acc[v, v] - c_a) - c_b
//     L[v, j] = L0[v, j] + acc[v, j] for every stored entry of the row, every acc starting at 0.0
//
// Both ends of an edge add the same products in the same order, so the revalued stiffness block is symmetric bit for bit; an
// edge the assembly did not store (both its weights exactly 0) takes a contribution of exactly 0 and is skipped.  Rows that
// are no vertex's are copied from L0.  With every s == 1 every product is 0 and L has the bits of L0.
//
// Kernels: memory-bound gathers and streams, workgroups of 256, no floating-point atomics; the largest change of a face
// mean is a maximum per 256-face tile and then one workgroup over the tiles, in the wave order of error.hpp.  Compiled
// with -ffp-contract=off: a numpy restatement reproduces every expression.
#include "thermal.hpp"

#include <cmath>
#include <vector>

namespace padne {                            // (struct padne_coupled: thermal.hpp)

constexpr unsigned long long kCoupledNoFace = ~0ULL;

__device__ __forceinline__ double coupled_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double coupled_max4(const double *red) {
    double v = red[0];
    for (int q = 1; q < 4; ++q) v = red[q] > v ? red[q] : v;
    return v;
}

// Per face: the mean of theta (null: the copper at ambient, mean 0), s, and |mean - prev| with prev <- mean; per tile of 256
// faces tile_d[b] = the largest of those.  A face whose 1 + alpha (T - T0) is not finite and positive posts its number to
// *bad_face (the lowest wins: an integer minimum)
__global__ __launch_bounds__(256) void coupled_scale_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                            const long long *__restrict__ voff, const long long *__restrict__ toff,
                                                            const double *__restrict__ alpha, const double ambient, const double t0,
                                                            const double *__restrict__ theta, double *__restrict__ prev,
                                                            double *__restrict__ s, double *__restrict__ tile_d,
                                                            unsigned long long *__restrict__ bad_face) {
    __shared__ double red[4];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    double d = 0.0;
    if (t < n_tri) {
        const int m = find_segment(toff, n_mesh, t);
        long long g1 = 0, g2 = 0, g3 = 0;
        const bool ok = error_corners(tri, voff, m, t, g1, g2, g3);      // (an index out of range was refused at creation)
        const double mean = theta != nullptr && ok ? ((theta[g1] + theta[g2]) + theta[g3]) / 3 : 0.0;
        const double den = 1 + alpha[m] * ((mean + ambient) - t0);
        if (!(den > 0.0) || !isfinite(den)) atomicMin(bad_face, (unsigned long long)t);
        s[t] = 1 / den;
        d = fabs(mean - prev[t]);
        prev[t] = mean;
    }
    d = coupled_wave_max(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) tile_d[blockIdx.x] = coupled_max4(red);
}

// out[0] = the largest tile_d, by one workgroup
__global__ __launch_bounds__(256) void coupled_fold_kernel(const long long n_tiles, const double *__restrict__ tile_d,
                                                           double *__restrict__ out) {
    __shared__ double red[4];
    double d = 0.0;
    for (long long i = threadIdx.x; i < n_tiles; i += 256) d = tile_d[i] > d ? tile_d[i] : d;
    d = coupled_wave_max(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = coupled_max4(red);
}

// the entry of column `col` among the ascending columns cols[e0 .. e1), or -1
__device__ __forceinline__ int coupled_find(const int32_t *__restrict__ cols, int e0, int e1, long long col) {
    while (e0 < e1) {
        const int mid = (e0 + e1) >> 1;
        const long long c = cols[mid];
        if (c == col) return mid;
        if (c < col) e0 = mid + 1; else e1 = mid;
    }
    return -1;
}

// The values of L from L0 and s, the expression at the top of this file.  One thread per row: the row's own entries of vals
// hold the accumulators between the two passes.  *err: a contribution that is not 0 has no stored entry to go to
__global__ __launch_bounds__(256) void coupled_revalue_kernel(const long long n_rows, const long long n_vert, const int n_mesh,
                                                              const int32_t *__restrict__ rowptr, const int32_t *__restrict__ cols,
                                                              const double *__restrict__ L0, double *__restrict__ vals,
                                                              const int32_t *__restrict__ tri, const double *__restrict__ xy,
                                                              const long long *__restrict__ voff, const long long *__restrict__ toff,
                                                              const double *__restrict__ sigma, const double *__restrict__ s,
                                                              const int *__restrict__ vptr, const int *__restrict__ vface,
                                                              int *__restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    if (i >= n_vert) {
        for (int e = e0; e < e1; ++e) vals[e] = L0[e];
        return;
    }
    for (int e = e0; e < e1; ++e) vals[e] = 0.0;
    const int at_d = coupled_find(cols, e0, e1, i);
    double acc_d = 0.0;
    for (int q = vptr[i], q1 = vptr[i + 1]; q < q1; ++q) {
        const long long t = vface[q];
        const int m = find_segment(toff, n_mesh, t);
        long long g1, g2, g3;
        if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
            *(volatile int *)err = 1;
            continue;
        }
        const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
        const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
        const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
        const double w23 = cot_half(x2, y2, x3, y3, x1, y1);
        const double w31 = cot_half(x3, y3, x1, y1, x2, y2);
        const double w12 = cot_half(x1, y1, x2, y2, x3, y3);
        const double tf = (s[t] - 1) * sigma[m];
        long long a, b;
        double wa, wb;
        if (i == g1) {
            a = g2; wa = w12; b = g3; wb = w31;
        } else if (i == g2) {
            a = g3; wa = w23; b = g1; wb = w12;
        } else {
            a = g1; wa = w31; b = g2; wb = w23;
        }
        const double ca = tf * wa, cb = tf * wb;
        const int at_a = coupled_find(cols, e0, e1, a), at_b = coupled_find(cols, e0, e1, b);
        if (at_a >= 0) vals[at_a] = vals[at_a] + ca;
        else if (ca != 0.0) *(volatile int *)err = 1;
        if (at_b >= 0) vals[at_b] = vals[at_b] + cb;
        else if (cb != 0.0) *(volatile int *)err = 1;
        acc_d = (acc_d - ca) - cb;
    }
    if (at_d >= 0) vals[at_d] = acc_d;
    else if (acc_d != 0.0) *(volatile int *)err = 1;
    for (int e = e0; e < e1; ++e) vals[e] = L0[e] + vals[e];
}

// p[t] = p[t] * s[t]: the power density sigma |grad V|^2 of power_density_block_kernel becomes that of the scaled face
__global__ __launch_bounds__(256) void coupled_post_scale_kernel(const long long n, const double *__restrict__ s,
                                                                 double *__restrict__ p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) p[t] = p[t] * s[t];
}

static int coupled_require(const char *entry, padne_ctx *ctx, const padne_coupled *cp) {
    PADNE_REQUIRE(ctx && cp, "null argument");
    PADNE_REQUIRE(cp->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    return PADNE_OK;
}

// what was derived from L's values: rebuilt on next use from the values in place
static void coupled_invalidate(padne_csr *L) { csr_invalidate_values(L); }

static void coupled_free(padne_coupled *cp) {
    if (cp == nullptr) return;
    padne_ctx *ctx = cp->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)cp->L0, (void *)cp->s, (void *)cp->s_used, (void *)cp->prev, (void *)cp->alpha})
        if (p != nullptr) pool_free(ctx, p);
    delete cp;
}

// the scale kernel and its fold on `theta` (device, null: zeros): *d_out (may be null) the largest change of a face mean;
// PADNE_E_INVALID names the lowest face whose scale is invalid
int coupled_run_scale(padne_ctx *ctx, padne_coupled *cp, const double *theta, double *d_out) {
    hipStream_t st = ctx->stream;
    if (d_out != nullptr) *d_out = 0.0;
    if (cp->n_tri == 0) return PADNE_OK;
    const ErrorMesh M = error_mesh_of(cp->L);
    const long long n_tiles = nblk(cp->n_tri);
    Scratch sc(ctx);
    double *d_tile = nullptr, *d_max = nullptr;
    unsigned long long *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_tile, (size_t)n_tiles));
    PADNE_TRY(sc.alloc(&d_max, 1));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(coupled_scale_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, cp->n_tri, cp->n_mesh, M.tri, M.voff, M.toff,
                       (const double *)cp->alpha, cp->ambient, cp->t0, theta, cp->prev, cp->s, d_tile, d_bad);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(coupled_fold_kernel, dim3(1), dim3(256), 0, st, n_tiles, (const double *)d_tile, d_max);
    PADNE_HIP_CHECK(hipGetLastError());
    double h_max = 0.0;
    unsigned long long h_bad = kCoupledNoFace;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_max, d_max, sizeof(double), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    if (h_bad != kCoupledNoFace) {
        set_error("invalid argument: 1 + alpha (T - T0) is not finite and positive on face %llu: the conductance model does not hold "
                  "at that temperature", h_bad);
        return PADNE_E_INVALID;
    }
    if (d_out != nullptr) *d_out = h_max;
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_coupled_create(padne_ctx *ctx, padne_csr *L, padne_thermal *th, int32_t n_mesh, const double *alpha,
                                    double ambient, double conductance_temperature, padne_coupled **out) {
    PADNE_REQUIRE(ctx && L && th && alpha && out, "null argument");
    PADNE_REQUIRE(th->ctx == ctx && th->L == L, "the thermal handle must come from this context and this system");
    PADNE_REQUIRE(L->owner == ctx, "the system must belong to this context");
    PADNE_REQUIRE(L->mesh_n_mesh > 0 && L->mesh_xy != nullptr, "the system matrix does not carry a mesh");
    PADNE_REQUIRE(n_mesh == L->mesh_n_mesh, "n_mesh must be that of the system's mesh");
    PADNE_REQUIRE(!L->cols_unsorted, "the columns of every row must ascend");
    PADNE_REQUIRE(L->nnz <= 0x7fffffffLL, "too many entries");
    PADNE_REQUIRE(std::isfinite(ambient) && std::isfinite(conductance_temperature), "the temperatures must be finite");
    for (int m = 0; m < n_mesh; ++m) PADNE_REQUIRE(std::isfinite(alpha[m]), "the temperature coefficient of every mesh must be finite");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    padne_coupled *cp = new padne_coupled;
    cp->ctx = ctx;
    cp->L = L;
    cp->th = th;
    cp->n_vert = L->mesh_n_vert;
    cp->n_tri = L->mesh_n_tri;
    cp->nnz = L->nnz;
    cp->n_mesh = n_mesh;
    cp->ambient = ambient;
    cp->t0 = conductance_temperature;
    struct Guard {
        padne_coupled *cp;
        ~Guard() { coupled_free(cp); }
    } guard{cp};
    const size_t nt = (size_t)(cp->n_tri > 0 ? cp->n_tri : 1), nz = (size_t)(cp->nnz > 0 ? cp->nnz : 1);
    cp->L0 = (double *)pool_alloc(ctx, sizeof(double) * nz);
    cp->s = (double *)pool_alloc(ctx, sizeof(double) * nt);
    cp->s_used = (double *)pool_alloc(ctx, sizeof(double) * nt);
    cp->prev = (double *)pool_alloc(ctx, sizeof(double) * nt);
    cp->alpha = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_mesh);
    if (!cp->L0 || !cp->s || !cp->s_used || !cp->prev || !cp->alpha) return PADNE_E_NOMEM;
    if (cp->nnz > 0) PADNE_HIP_CHECK(hipMemcpyAsync(cp->L0, L->vals, sizeof(double) * (size_t)cp->nnz, hipMemcpyDeviceToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(cp->alpha, alpha, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemsetAsync(cp->prev, 0, sizeof(double) * nt, st));
    PADNE_TRY(coupled_run_scale(ctx, cp, nullptr, nullptr));        // s^(0): the copper at ambient (synchronises: alpha may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(cp->s_used, cp->s, sizeof(double) * nt, hipMemcpyDeviceToDevice, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    guard.cp = nullptr;
    *out = cp;
    return PADNE_OK;
}

extern "C" int padne_coupled_destroy(padne_coupled *cp) {
    if (cp == nullptr) return PADNE_OK;
    padne_ctx *ctx = cp->ctx;
    int rc = PADNE_OK;
    if (ctx != nullptr && cp->L != nullptr && cp->L0 != nullptr && cp->nnz > 0) {
        (void)hipSetDevice(ctx->device);
        coupled_invalidate(cp->L);
        if (hipMemcpyAsync(cp->L->vals, cp->L0, sizeof(double) * (size_t)cp->nnz, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            set_error("padne_coupled_destroy: the assembled values could not be restored");
            rc = PADNE_E_HIP;
        }
    }
    coupled_free(cp);
    return rc;
}

extern "C" int padne_coupled_reset(padne_ctx *ctx, padne_coupled *cp) {
    PADNE_TRY(coupled_require("padne_coupled_reset", ctx, cp));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemsetAsync(cp->prev, 0, sizeof(double) * (size_t)(cp->n_tri > 0 ? cp->n_tri : 1), ctx->stream));
    return coupled_run_scale(ctx, cp, nullptr, nullptr);
}

extern "C" int padne_coupled_set_scale(padne_ctx *ctx, padne_coupled *cp, int64_t n_tri, const double *scale_host) {
    PADNE_TRY(coupled_require("padne_coupled_set_scale", ctx, cp));
    PADNE_REQUIRE(n_tri == cp->n_tri, "n_tri must be that of the system's mesh");
    if (n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(scale_host != nullptr, "null argument");
    for (int64_t t = 0; t < n_tri; ++t) PADNE_REQUIRE(std::isfinite(scale_host[t]) && scale_host[t] > 0.0, "a scale must be finite and positive");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(cp->s, scale_host, sizeof(double) * (size_t)n_tri, hipMemcpyHostToDevice, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_coupled_get_scale(padne_ctx *ctx, const padne_coupled *cp, int32_t used, int64_t n_tri, double *scale_out,
                                       double *face_mean_out) {
    PADNE_TRY(coupled_require("padne_coupled_get_scale", ctx, cp));
    PADNE_REQUIRE(n_tri == cp->n_tri, "n_tri must be that of the system's mesh");
    PADNE_REQUIRE(used == 0 || used == 1, "used is 0 (the next revalue's scale) or 1 (the last one's)");
    if (n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(scale_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(scale_out, used ? cp->s_used : cp->s, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, ctx->stream));
    if (face_mean_out != nullptr)
        PADNE_HIP_CHECK(hipMemcpyAsync(face_mean_out, cp->prev, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_coupled_revalue(padne_ctx *ctx, padne_coupled *cp) {
    PADNE_TRY(coupled_require("padne_coupled_revalue", ctx, cp));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    padne_csr *L = cp->L;
    PADNE_REQUIRE(!L->cols_unsorted, "the columns of every row must ascend");
    coupled_invalidate(L);
    if (cp->n_tri > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(cp->s_used, cp->s, sizeof(double) * (size_t)cp->n_tri, hipMemcpyDeviceToDevice, st));
    if (L->n_rows == 0) return PADNE_OK;
    const ErrorMesh M = error_mesh_of(L);
    Scratch sc(ctx);
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), st));
    hipLaunchKernelGGL(coupled_revalue_kernel, dim3(nblk(L->n_rows)), dim3(256), 0, st, (long long)L->n_rows, cp->n_vert, cp->n_mesh,
                       (const int32_t *)L->rowptr, (const int32_t *)L->cols, (const double *)cp->L0, L->vals, M.tri, M.xy, M.voff, M.toff,
                       M.sigma, (const double *)cp->s_used, (const int *)cp->th->vptr, (const int *)cp->th->vface, d_bad);
    PADNE_HIP_CHECK(hipGetLastError());
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    if (h_bad) {
        set_error("invalid argument: a face's contribution has no stored entry in the system (is this the system the mesh was assembled into?)");
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}

extern "C" int padne_coupled_update(padne_ctx *ctx, padne_coupled *cp, int64_t n_theta, const double *theta_host, double *increment_out) {
    PADNE_TRY(coupled_require("padne_coupled_update", ctx, cp));
    PADNE_REQUIRE(increment_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const padne_thermal *th = cp->th;
    if (theta_host == nullptr) {
        PADNE_REQUIRE(th->solved && th->n_cols == 1, "padne_coupled_update follows a thermal solve of one column");
        return coupled_run_scale(ctx, cp, th->theta, increment_out);
    }
    PADNE_REQUIRE(n_theta == th->n_pot, "theta has one entry per potential unknown");
    for (int64_t i = 0; i < n_theta; ++i) PADNE_REQUIRE(std::isfinite(theta_host[i]), "theta must be finite");
    Scratch sc(ctx);
    double *d_theta = nullptr;
    PADNE_TRY(sc.alloc(&d_theta, (size_t)n_theta));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_theta, theta_host, sizeof(double) * (size_t)n_theta, hipMemcpyHostToDevice, ctx->stream));
    return coupled_run_scale(ctx, cp, d_theta, increment_out);
}

extern "C" int padne_coupled_solve_kkt(padne_ctx *ctx, padne_coupled *cp, padne_kkt *plan, int64_t n_heat, const int64_t *heat_node,
                                       const int32_t *heat_col, const double *heat_val, const padne_solve_opts *opts,
                                       double *theta_host, padne_solve_info *info) {
    PADNE_TRY(coupled_require("padne_coupled_solve_kkt", ctx, cp));
    return thermal_solve_kkt_scaled("padne_coupled_solve_kkt", ctx, cp->th, plan, 1, cp->s_used, n_heat, heat_node, heat_col, heat_val,
                                    opts, theta_host, info);
}

extern "C" int padne_coupled_power_density(padne_ctx *ctx, padne_coupled *cp, padne_kkt *plan, double *out_host) {
    PADNE_TRY(coupled_require("padne_coupled_power_density", ctx, cp));
    const double *V = nullptr;
    long long N = 0;
    const padne_csr *L = nullptr;
    PADNE_TRY(kkt_finished_block("padne_coupled_power_density", ctx, plan, 1, &V, &N, &L));
    PADNE_REQUIRE(L == cp->L, "the plan and the coupling must come from the same assembled system");
    if (cp->n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(out_host != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    double *d_out = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_out, (size_t)cp->n_tri));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), st));
    PADNE_TRY(launch_power_density_block(ctx, L, 1, V, d_out, d_bad));
    hipLaunchKernelGGL(coupled_post_scale_kernel, dim3(nblk(cp->n_tri)), dim3(256), 0, st, cp->n_tri, (const double *)cp->s_used, d_out);
    PADNE_HIP_CHECK(hipGetLastError());
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, sizeof(double) * (size_t)cp->n_tri, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    PADNE_REQUIRE(!h_bad, "triangle index out of range");
    return PADNE_OK;
}
