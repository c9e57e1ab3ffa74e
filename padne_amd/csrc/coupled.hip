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
// Lumped resistors whose resistance follows their temperature (padne_coupled_set_resistors; DESIGN.md, "Resistor coupling").
// Resistor r between the unknowns a_r and b_r (vertices or internal nodes) conducts g_r s_r, g_r = 1 / R_r, with
//
//     mean_r = (theta[a_r] + theta[b_r]) / 2,    s_r = 1 / (1 + alpha_r * ((mean_r + ambient) - t0_r))
//
// and the revalue above is followed, per row i that a resistor touches, by
//
//     for every resistor r at i (ascending r, those with a_r == b_r left out), j its other end, t_r = (s_r - 1) * g_r,
//         unless t_r == 0.0:   L[i, j] = L[i, j] + t_r;   L[i, i] = L[i, i] - t_r
//
// as sequential rounded updates of the stored values.  Both ends of a resistor apply the same operations in the same order
// to values that were equal bit for bit, so the potential block stays symmetric bit for bit, and with every s_r == 1 nothing
// is written.  Without resistors no kernel of theirs is launched and every entry does what it did before they existed.
//
// Kernels: memory-bound gathers and streams, workgroups of 256, no floating-point atomics; the largest change of a face
// mean is a maximum per 256-face tile and then one workgroup over the tiles, in the wave order of error.hpp, and the
// resistors' largest change likewise (two small launches behind the face pass, one behind the revalue: thousands of
// resistors, bound by launch latency).  Compiled with -ffp-contract=off: a numpy restatement reproduces every expression.
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

// Per resistor r with its ends at the unknowns a[r], b[r]: mean = (theta[a] + theta[b]) / 2 (theta null: 0), s[r] =
// 1 / (1 + alpha[r] * ((mean + ambient) - t0[r])) and |mean - prev[r]| with prev <- mean; per tile of 256 resistors tile_d[b]
// = the largest of those.  An invalid 1 + alpha (T - T0) posts the resistor's number to *bad_res (the lowest wins)
__global__ __launch_bounds__(256) void coupled_resistor_scale_kernel(const long long n_res, const int *__restrict__ a,
                                                                     const int *__restrict__ b, const double *__restrict__ alpha,
                                                                     const double ambient, const double *__restrict__ t0,
                                                                     const double *__restrict__ theta, double *__restrict__ prev,
                                                                     double *__restrict__ s, double *__restrict__ tile_d,
                                                                     unsigned long long *__restrict__ bad_res) {
    __shared__ double red[4];
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    double d = 0.0;
    if (r < n_res) {
        const double mean = theta != nullptr ? (theta[a[r]] + theta[b[r]]) / 2 : 0.0;
        const double den = 1 + alpha[r] * ((mean + ambient) - t0[r]);
        if (!(den > 0.0) || !isfinite(den)) atomicMin(bad_res, (unsigned long long)r);
        s[r] = 1 / den;
        d = fabs(mean - prev[r]);
        prev[r] = mean;
    }
    d = coupled_wave_max(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) tile_d[blockIdx.x] = coupled_max4(red);
}

// Setup: per incidence k of row inc_row[k] with the other end inc_col[k], the places in the values of that row's entry in
// column inc_col[k] and of its diagonal.  *err: an entry is not stored
__global__ __launch_bounds__(256) void coupled_resistor_places_kernel(const long long n_inc, const int *__restrict__ inc_row,
                                                                      const int *__restrict__ inc_col,
                                                                      const int32_t *__restrict__ rowptr,
                                                                      const int32_t *__restrict__ cols, int *__restrict__ at_other,
                                                                      int *__restrict__ at_diag, int *__restrict__ err) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_inc) return;
    const int i = inc_row[k];
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const int o = coupled_find(cols, e0, e1, inc_col[k]), d = coupled_find(cols, e0, e1, i);
    if (o < 0 || d < 0) *(volatile int *)err = 1;
    at_other[k] = o < 0 ? e0 : o;
    at_diag[k] = d < 0 ? e0 : d;
}

// The resistors' share of the revalue, behind coupled_revalue_kernel: one thread per touched row, its incidences in
// ascending resistor number, t_r = (s_r - 1) * g_r added to the entry in the other end's column and taken from the diagonal
// as sequential rounded updates of the stored values; t_r == 0.0 writes nothing.  A row's entries are its thread's alone
__global__ __launch_bounds__(256) void coupled_resistor_revalue_kernel(const long long n_rrow, const int *__restrict__ rr_ptr,
                                                                       const int *__restrict__ rr_res,
                                                                       const int *__restrict__ rr_other,
                                                                       const int *__restrict__ rr_diag, const double *__restrict__ s,
                                                                       const double *__restrict__ g, double *__restrict__ vals) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_rrow) return;
    for (int k = rr_ptr[q], k1 = rr_ptr[q + 1]; k < k1; ++k) {
        const int r = rr_res[k];
        const double t = (s[r] - 1) * g[r];
        if (t == 0.0) continue;
        vals[rr_other[k]] = vals[rr_other[k]] + t;
        vals[rr_diag[k]] = vals[rr_diag[k]] - t;
    }
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

// the resistors' arrays back to the pool (nothing queued may still use them)
static void coupled_drop_resistors(padne_coupled *cp) {
    for (void *p : {(void *)cp->r_a, (void *)cp->r_b, (void *)cp->r_g, (void *)cp->r_alpha, (void *)cp->r_t0, (void *)cp->r_s,
                    (void *)cp->r_s_used, (void *)cp->r_prev, (void *)cp->rr_ptr, (void *)cp->rr_res, (void *)cp->rr_other,
                    (void *)cp->rr_diag})
        if (p != nullptr) pool_free(cp->ctx, p);
    cp->r_a = cp->r_b = cp->rr_ptr = cp->rr_res = cp->rr_other = cp->rr_diag = nullptr;
    cp->r_g = cp->r_alpha = cp->r_t0 = cp->r_s = cp->r_s_used = cp->r_prev = nullptr;
    cp->n_res = cp->n_rrow = cp->n_inc = 0;
}

static void coupled_free(padne_coupled *cp) {
    if (cp == nullptr) return;
    padne_ctx *ctx = cp->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)cp->L0, (void *)cp->s, (void *)cp->s_used, (void *)cp->prev, (void *)cp->alpha})
        if (p != nullptr) pool_free(ctx, p);
    coupled_drop_resistors(cp);
    delete cp;
}

// the scale kernel and its fold on `theta` (device, null: zeros): *d_out (may be null) the largest change of a face mean;
// PADNE_E_INVALID names the lowest face whose scale is invalid
// With resistors set the resistor pass follows the face pass (two more launches) and *d_out is the larger of the two
// increments; an invalid face is reported before an invalid resistor.  `faces` false: the resistor pass alone
static int coupled_scale_pass(padne_ctx *ctx, padne_coupled *cp, const double *theta, double *d_out, bool faces) {
    hipStream_t st = ctx->stream;
    if (d_out != nullptr) *d_out = 0.0;
    const bool do_faces = faces && cp->n_tri > 0, do_res = cp->n_res > 0;
    if (!do_faces && !do_res) return PADNE_OK;
    Scratch sc(ctx);
    double *d_max = nullptr;
    unsigned long long *d_bad = nullptr;
    double h_max[2] = {0.0, 0.0};
    unsigned long long h_bad[2] = {kCoupledNoFace, kCoupledNoFace};
    if (do_faces) {
        const ErrorMesh M = error_mesh_of(cp->L);
        const long long n_tiles = nblk(cp->n_tri);
        double *d_tile = nullptr;
        PADNE_TRY(sc.alloc(&d_tile, (size_t)n_tiles));
        PADNE_TRY(sc.alloc(&d_max, 1));
        PADNE_TRY(sc.alloc(&d_bad, 1));
        PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(coupled_scale_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, cp->n_tri, cp->n_mesh, M.tri, M.voff,
                           M.toff, (const double *)cp->alpha, cp->ambient, cp->t0, theta, cp->prev, cp->s, d_tile, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(coupled_fold_kernel, dim3(1), dim3(256), 0, st, n_tiles, (const double *)d_tile, d_max);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    double *d_rmax = nullptr;
    unsigned long long *d_rbad = nullptr;
    if (do_res) {
        const long long n_tiles = nblk(cp->n_res);
        double *d_tile = nullptr;
        PADNE_TRY(sc.alloc(&d_tile, (size_t)n_tiles));
        PADNE_TRY(sc.alloc(&d_rmax, 1));
        PADNE_TRY(sc.alloc(&d_rbad, 1));
        PADNE_HIP_CHECK(hipMemsetAsync(d_rbad, 0xff, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(coupled_resistor_scale_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, cp->n_res, (const int *)cp->r_a,
                           (const int *)cp->r_b, (const double *)cp->r_alpha, cp->ambient, (const double *)cp->r_t0, theta, cp->r_prev,
                           cp->r_s, d_tile, d_rbad);
        PADNE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(coupled_fold_kernel, dim3(1), dim3(256), 0, st, n_tiles, (const double *)d_tile, d_rmax);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (do_faces) {                                     // (the copies behind every launch: none waits between two kernels)
        PADNE_HIP_CHECK(hipMemcpyAsync(&h_max[0], d_max, sizeof(double), hipMemcpyDeviceToHost, st));
        PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad[0], d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    if (do_res) {
        PADNE_HIP_CHECK(hipMemcpyAsync(&h_max[1], d_rmax, sizeof(double), hipMemcpyDeviceToHost, st));
        PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad[1], d_rbad, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    if (h_bad[0] != kCoupledNoFace) {
        set_error("invalid argument: 1 + alpha (T - T0) is not finite and positive on face %llu: the conductance model does not hold "
                  "at that temperature", h_bad[0]);
        return PADNE_E_INVALID;
    }
    if (h_bad[1] != kCoupledNoFace) {
        set_error("invalid argument: 1 + alpha (T - T0) is not finite and positive on resistor %llu: the resistance model does not "
                  "hold at that temperature", h_bad[1]);
        return PADNE_E_INVALID;
    }
    if (d_out != nullptr) *d_out = h_max[1] > h_max[0] ? h_max[1] : h_max[0];
    return PADNE_OK;
}

int coupled_run_scale(padne_ctx *ctx, padne_coupled *cp, const double *theta, double *d_out) {
    return coupled_scale_pass(ctx, cp, theta, d_out, true);
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
    if (cp->n_res > 0) PADNE_HIP_CHECK(hipMemsetAsync(cp->r_prev, 0, sizeof(double) * (size_t)cp->n_res, ctx->stream));
    return coupled_run_scale(ctx, cp, nullptr, nullptr);
}

extern "C" int padne_coupled_set_resistors(padne_ctx *ctx, padne_coupled *cp, int64_t n_res, const int64_t *a, const int64_t *b,
                                           const double *R, const double *alpha, const double *t0) {
    PADNE_TRY(coupled_require("padne_coupled_set_resistors", ctx, cp));
    PADNE_REQUIRE(n_res >= 0 && n_res <= 0x3fffffffLL, "the number of resistors is out of range");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n_res == 0) {
        PADNE_HIP_CHECK(hipStreamSynchronize(st));
        coupled_drop_resistors(cp);
        return PADNE_OK;
    }
    PADNE_REQUIRE(a && b && R && alpha && t0, "null argument");
    const padne_csr *L = cp->L;
    const long long n_pot = cp->th->n_pot;
    PADNE_REQUIRE(n_pot <= L->n_rows, "the system has fewer rows than the thermal handle has potential unknowns");
    const size_t n = (size_t)n_res;
    std::vector<int> h_a(n), h_b(n);
    std::vector<double> h_g(n);
    for (size_t r = 0; r < n; ++r) {
        PADNE_REQUIRE(a[r] >= 0 && a[r] < n_pot && b[r] >= 0 && b[r] < n_pot, "an end of a resistor is no potential unknown");
        PADNE_REQUIRE(std::isfinite(R[r]) && R[r] > 0.0, "a resistance must be finite and positive");
        PADNE_REQUIRE(std::isfinite(alpha[r]) && std::isfinite(t0[r]), "the temperature coefficient and T0 of every resistor must be finite");
        const double den = 1 + alpha[r] * ((0.0 + cp->ambient) - t0[r]);
        if (!(den > 0.0) || !std::isfinite(den)) {
            set_error("invalid argument: 1 + alpha (T - T0) is not finite and positive on resistor %llu at the ambient temperature",
                      (unsigned long long)r);
            return PADNE_E_INVALID;
        }
        h_a[r] = (int)a[r];
        h_b[r] = (int)b[r];
        h_g[r] = 1 / R[r];
    }
    // unknown -> resistors as CSR over the touched rows: a counting sort by row keeps the resistors of a row ascending
    std::vector<int> count((size_t)n_pot + 1, 0);
    for (size_t r = 0; r < n; ++r)
        if (h_a[r] != h_b[r]) {
            ++count[(size_t)h_a[r] + 1];
            ++count[(size_t)h_b[r] + 1];
        }
    for (long long i = 0; i < n_pot; ++i) count[(size_t)i + 1] += count[(size_t)i];
    const size_t n_inc = (size_t)count[(size_t)n_pot];
    std::vector<int> h_ptr(1, 0), inc_row(n_inc), inc_col(n_inc), inc_res(n_inc), fill(count.begin(), count.end() - 1);
    for (size_t r = 0; r < n; ++r)
        if (h_a[r] != h_b[r]) {
            const int ka = fill[(size_t)h_a[r]]++, kb = fill[(size_t)h_b[r]]++;
            inc_row[(size_t)ka] = h_a[r]; inc_col[(size_t)ka] = h_b[r]; inc_res[(size_t)ka] = (int)r;
            inc_row[(size_t)kb] = h_b[r]; inc_col[(size_t)kb] = h_a[r]; inc_res[(size_t)kb] = (int)r;
        }
    for (long long i = 0; i < n_pot; ++i)
        if (count[(size_t)i + 1] > count[(size_t)i]) h_ptr.push_back(count[(size_t)i + 1]);
    const size_t n_rrow = h_ptr.size() - 1;
    // the new arrays, complete before they replace the handle's
    Scratch sc(ctx);
    int *d_a = nullptr, *d_b = nullptr, *d_ptr = nullptr, *d_res = nullptr, *d_other = nullptr, *d_diag = nullptr, *d_row = nullptr,
        *d_col = nullptr, *d_err = nullptr;
    double *d_g = nullptr, *d_alpha = nullptr, *d_t0 = nullptr, *d_s = nullptr, *d_su = nullptr, *d_prev = nullptr;
    PADNE_TRY(sc.alloc(&d_a, n));
    PADNE_TRY(sc.alloc(&d_b, n));
    PADNE_TRY(sc.alloc(&d_g, n));
    PADNE_TRY(sc.alloc(&d_alpha, n));
    PADNE_TRY(sc.alloc(&d_t0, n));
    PADNE_TRY(sc.alloc(&d_s, n));
    PADNE_TRY(sc.alloc(&d_su, n));
    PADNE_TRY(sc.alloc(&d_prev, n));
    PADNE_TRY(sc.alloc(&d_ptr, n_rrow + 1));
    PADNE_TRY(sc.alloc(&d_res, n_inc));
    PADNE_TRY(sc.alloc(&d_other, n_inc));
    PADNE_TRY(sc.alloc(&d_diag, n_inc));
    PADNE_TRY(sc.alloc(&d_row, n_inc));
    PADNE_TRY(sc.alloc(&d_col, n_inc));
    PADNE_TRY(sc.alloc(&d_err, 1));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_a, h_a.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_b, h_b.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_g, h_g.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_alpha, alpha, sizeof(double) * n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_t0, t0, sizeof(double) * n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ptr, h_ptr.data(), sizeof(int) * (n_rrow + 1), hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemsetAsync(d_prev, 0, sizeof(double) * n, st));
    PADNE_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), st));
    int h_err = 0;
    if (n_inc > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_res, inc_res.data(), sizeof(int) * n_inc, hipMemcpyHostToDevice, st));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_row, inc_row.data(), sizeof(int) * n_inc, hipMemcpyHostToDevice, st));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_col, inc_col.data(), sizeof(int) * n_inc, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(coupled_resistor_places_kernel, dim3(nblk((long long)n_inc)), dim3(256), 0, st, (long long)n_inc,
                           (const int *)d_row, (const int *)d_col, (const int32_t *)L->rowptr, (const int32_t *)L->cols, d_other,
                           d_diag, d_err);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(st));          // (the host arrays may go; nothing queued uses the old arrays)
    if (h_err) {
        set_error("invalid argument: a resistor's stamp has no stored entry in the system (is this the system the resistors were "
                  "assembled into?)");
        return PADNE_E_INVALID;
    }
    coupled_drop_resistors(cp);
    for (void *p : {(void *)d_a, (void *)d_b, (void *)d_g, (void *)d_alpha, (void *)d_t0, (void *)d_s, (void *)d_su, (void *)d_prev,
                    (void *)d_ptr, (void *)d_res, (void *)d_other, (void *)d_diag})
        sc.disown(p);
    cp->r_a = d_a; cp->r_b = d_b; cp->r_g = d_g; cp->r_alpha = d_alpha; cp->r_t0 = d_t0;
    cp->r_s = d_s; cp->r_s_used = d_su; cp->r_prev = d_prev;
    cp->rr_ptr = d_ptr; cp->rr_res = d_res; cp->rr_other = d_other; cp->rr_diag = d_diag;
    cp->n_res = n_res; cp->n_rrow = (long long)n_rrow; cp->n_inc = (long long)n_inc;
    // s, s_used and prev of the resistors at ambient (valid there: checked above)
    PADNE_TRY(coupled_scale_pass(ctx, cp, nullptr, nullptr, false));
    PADNE_HIP_CHECK(hipMemcpyAsync(cp->r_s_used, cp->r_s, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    return PADNE_OK;
}

extern "C" int padne_coupled_get_resistors(padne_ctx *ctx, const padne_coupled *cp, int32_t used, int64_t n_res, double *scale_out,
                                           double *mean_out) {
    PADNE_TRY(coupled_require("padne_coupled_get_resistors", ctx, cp));
    PADNE_REQUIRE(n_res == cp->n_res, "n_res must be the number of resistors set");
    PADNE_REQUIRE(used == 0 || used == 1, "used is 0 (the next revalue's scale) or 1 (the last one's)");
    if (n_res == 0) return PADNE_OK;
    PADNE_REQUIRE(scale_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(scale_out, used ? cp->r_s_used : cp->r_s, sizeof(double) * (size_t)n_res, hipMemcpyDeviceToHost, ctx->stream));
    if (mean_out != nullptr)
        PADNE_HIP_CHECK(hipMemcpyAsync(mean_out, cp->r_prev, sizeof(double) * (size_t)n_res, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
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
    coupled_invalidate(L);
    if (cp->n_tri > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(cp->s_used, cp->s, sizeof(double) * (size_t)cp->n_tri, hipMemcpyDeviceToDevice, st));
    if (cp->n_res > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(cp->r_s_used, cp->r_s, sizeof(double) * (size_t)cp->n_res, hipMemcpyDeviceToDevice, st));
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
    if (cp->n_rrow > 0) {
        hipLaunchKernelGGL(coupled_resistor_revalue_kernel, dim3(nblk(cp->n_rrow)), dim3(256), 0, st, cp->n_rrow,
                           (const int *)cp->rr_ptr, (const int *)cp->rr_res, (const int *)cp->rr_other, (const int *)cp->rr_diag,
                           (const double *)cp->r_s_used, (const double *)cp->r_g, L->vals);
        PADNE_HIP_CHECK(hipGetLastError());
    }
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
