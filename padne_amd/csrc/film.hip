// Film coefficients that depend on the temperature rise, by Newton rounds ("Film curves").  No reference counterpart.
//
// The film of mesh m is a table: h = film[i] at the knots rise[i] [K above ambient], linear between them, held constant below
// the first knot (rise[0] == 0) and above the last.  The loss density q(theta) = h(theta) theta is strictly increasing (checked
// when the tables are given), so the balance film loss = heat put in has one steady state and Newton's linearisation keeps
// the matrix the M-matrix the multigrid path solves.  About an iterate theta, vertex v of mesh m uses the segment i that
// contains theta[v] -- the largest i with rise[i] <= theta[v], found by a fixed-trip binary search -- with its slope
// s = (film[i + 1] - film[i]) / (rise[i + 1] - rise[i]) (formed once on the host when the tables are given), s = 0 in both
// clamped ranges, and
//
//     h    = film[i] + s * (theta - rise[i])          g = h + s * theta                     (g = q'(theta))
//     d_v  = g * M_v                                  the film's diagonal for the round
//     c_v  = ((s * theta) * theta) * M_v              added to the load: (q'(theta) theta - q(theta)) M_v
//     hM_v = h * M_v                                  what the reports multiply theta by
//
// The round solves (A - diag(hM0) + diag(d)) theta' = b + c from theta: the stored diagonal of vertex v becomes the one
// rounded sum D0_v + (d_v - hM0_v), D0 and hM0 = film[0] M_v what the create call left.  At theta = 0, and for a table of one
// knot at any theta, d_v has the bits of hM0_v and c_v is 0: the diagonal keeps its bits, a zero column stays exact zeros.
//
// One kernel serves the three passes (the terms alone, the linearisation, the increment): one thread per vertex in tiles of
// 256 vertices of one mesh (thermal_tiles over voff, as the report kernels), the mesh's table staged in LDS once per
// workgroup, about 76 bytes per vertex.  The (value, vertex) top and the count of vertices above their last knot go through
// the fixed two-level order of error.hpp; no floating-point atomics: two calls give the same bits.  Compiled with
// -ffp-contract=off, + - * only on the device: a numpy restatement reproduces every bit.
#include "thermal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace padne {

constexpr int kFilmKnots = 64;               // the most knots of one table

__device__ __forceinline__ long long film_wave_count(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// diag[v] = the entry of row v that holds its diagonal (-1: none; the create call refused such a row), D0[v] its value
__global__ __launch_bounds__(256) void film_diag_kernel(const long long n_vert, const int32_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                        int *__restrict__ diag, double *__restrict__ D0, int *__restrict__ err) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    int at = -1;
    for (int e = rowptr[v], e1 = rowptr[v + 1]; e < e1; ++e)
        if (cols[e] == v) at = e;
    diag[v] = at;
    D0[v] = at >= 0 ? vals[at] : 0.0;
    if (at < 0) *(volatile int *)err = 1;
}

// vals[diag[v]] = D0[v], the diagonal of the create call
__global__ __launch_bounds__(256) void film_restore_kernel(const long long n_vert, const int *__restrict__ diag,
                                                           const double *__restrict__ D0, double *__restrict__ vals) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vert) vals[diag[v]] = D0[v];
}

// b[v] = b[v] + c[v]
__global__ __launch_bounds__(256) void film_add_kernel(const long long n_vert, const double *__restrict__ c, double *__restrict__ b) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vert) b[v] = b[v] + c[v];
}

// The terms of the file's head at theta (null: zeros) for every vertex of a tile.  What is not null is written: g_out, c_out
// and hM_out per vertex; vals, the stored diagonal through diag (with D0 and hM0); per tile the largest |theta - lin| with
// its vertex (the lowest on a tie) in tile_inc / tile_vert and the number of vertices above the last knot of a table of
// more than one knot in tile_beyond
__global__ __launch_bounds__(256) void film_terms_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                         const long long *__restrict__ voff, const int *__restrict__ kptr,
                                                         const double *__restrict__ krise, const double *__restrict__ kfilm,
                                                         const double *__restrict__ kslope, const double *__restrict__ Mv,
                                                         const double *__restrict__ theta, const double *__restrict__ lin,
                                                         double *__restrict__ g_out, double *__restrict__ c_out,
                                                         double *__restrict__ hM_out, const int *__restrict__ diag,
                                                         const double *__restrict__ D0, const double *__restrict__ hM0,
                                                         double *__restrict__ vals, double *__restrict__ tile_inc,
                                                         long long *__restrict__ tile_vert, long long *__restrict__ tile_beyond) {
    __shared__ double t_s[kFilmKnots], h_s[kFilmKnots], s_s[kFilmKnots];
    __shared__ double red_v[4];
    __shared__ long long red_f[4], red_n[4];
    const long long b = blockIdx.x;
    const int m = find_segment(vtile_off, n_mesh, b);
    const int k0 = kptr[m], nk = kptr[m + 1] - k0;      // 1 <= nk <= kFilmKnots (checked when the tables were given)
    if (threadIdx.x < kFilmKnots) {
        const bool in = (int)threadIdx.x < nk;
        t_s[threadIdx.x] = in ? krise[k0 + threadIdx.x] : INFINITY;
        h_s[threadIdx.x] = in ? kfilm[k0 + threadIdx.x] : 0.0;
        s_s[threadIdx.x] = in ? kslope[k0 + threadIdx.x] : 0.0;
    }
    __syncthreads();
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    const bool live = v < voff[m + 1];
    double a = -INFINITY;
    long long f = kErrNoFace, beyond = 0;
    if (live) {
        const double th = theta != nullptr ? theta[v] : 0.0;
        int i = 0;
#pragma unroll
        for (int step = kFilmKnots / 2; step > 0; step >>= 1) {
            const int cand = i + step;
            if (cand < nk && t_s[cand] <= th) i = cand;
        }
        // below the first knot (and for a NaN) the table's first value holds; kslope is 0 at the last knot
        const double s = th >= t_s[0] ? s_s[i] : 0.0;
        const double h = h_s[i] + s * (th - t_s[i]);
        const double g = h + s * th;
        const double mv = Mv[v];
        if (g_out != nullptr) g_out[v] = g;
        if (c_out != nullptr) c_out[v] = ((s * th) * th) * mv;
        if (hM_out != nullptr) hM_out[v] = h * mv;
        if (vals != nullptr) vals[diag[v]] = D0[v] + (g * mv - hM0[v]);
        if (nk > 1 && th > t_s[nk - 1]) beyond = 1;
        if (tile_inc != nullptr) {
            a = fabs(th - lin[v]);
            f = v;
        }
    }
    if (tile_inc == nullptr && tile_beyond == nullptr) return;      // (uniform over the grid)
    error_wave_top(a, f);
    beyond = film_wave_count(beyond);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
        red_n[threadIdx.x >> 6] = beyond;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        if (tile_inc != nullptr) {
            tile_inc[b] = a;
            tile_vert[b] = f;
        }
        if (tile_beyond != nullptr) tile_beyond[b] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
    }
}

// over all tiles by one workgroup, strided partial results and then the order of error.hpp: out_inc[0] / out_vert[0] the
// largest tile_inc with its vertex (tile_inc null: not written; -infinity and kErrNoFace without tiles), out_beyond[0] the
// sum of tile_beyond
__global__ __launch_bounds__(256) void film_fold_kernel(const long long n_tiles, const double *__restrict__ tile_inc,
                                                        const long long *__restrict__ tile_vert,
                                                        const long long *__restrict__ tile_beyond, double *__restrict__ out_inc,
                                                        long long *__restrict__ out_vert, long long *__restrict__ out_beyond) {
    __shared__ double red_v[4];
    __shared__ long long red_f[4], red_n[4];
    double a = -INFINITY;
    long long f = kErrNoFace, n = 0;
    for (long long i = threadIdx.x; i < n_tiles; i += 256) {
        if (tile_inc != nullptr) error_merge(a, f, tile_inc[i], tile_vert[i]);
        n += tile_beyond[i];
    }
    error_wave_top(a, f);
    n = film_wave_count(n);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
        red_n[threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        if (tile_inc != nullptr) {
            out_inc[0] = a;
            out_vert[0] = f;
        }
        out_beyond[0] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
    }
}

void film_free(padne_ctx *ctx, padne_film *fm) {
    if (fm == nullptr) return;
    for (void *p : {(void *)fm->kptr, (void *)fm->krise, (void *)fm->kfilm, (void *)fm->kslope, (void *)fm->diag, (void *)fm->D0,
                    (void *)fm->hM0, (void *)fm->c, (void *)fm->lin, (void *)fm->b0})
        if (p != nullptr) pool_free(ctx, p);
    delete fm;
}

int film_refuses(const char *entry, const padne_thermal *th, int32_t n_cols) {
    if (th->film != nullptr && n_cols != 1) {
        set_error("invalid argument: %s: a handle with film curves solves one column at a time, not %d", entry, (int)n_cols);
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}

int film_add_load(padne_ctx *ctx, padne_thermal *th, double *d_b) {
    if (th->film == nullptr || th->n_vert == 0) return PADNE_OK;
    hipLaunchKernelGGL(film_add_kernel, dim3(nblk(th->n_vert)), dim3(256), 0, ctx->stream, th->n_vert, (const double *)th->film->c, d_b);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

// what check_film_curve refuses of one table of nk knots; *slope[nk] the segments' slopes, 0 at the last knot
static int film_check_table(int m, int nk, const double *rise, const double *film, double *slope) {
    if (nk < 1 || nk > kFilmKnots) {
        set_error("invalid argument: the film curve of mesh %d has %d knots: between 1 and %d are taken", m, nk, kFilmKnots);
        return PADNE_E_INVALID;
    }
    for (int i = 0; i < nk; ++i) {
        if (!std::isfinite(rise[i]) || !std::isfinite(film[i]) || !(film[i] > 0.0)) {
            set_error("invalid argument: the film curve of mesh %d: knot %d must be finite with a positive film coefficient", m, i);
            return PADNE_E_INVALID;
        }
        if (i == 0 ? rise[0] != 0.0 : !(rise[i] > rise[i - 1])) {
            set_error("invalid argument: the film curve of mesh %d: the rises must start at 0 and ascend strictly (knot %d)", m, i);
            return PADNE_E_INVALID;
        }
    }
    for (int i = 0; i < nk; ++i) slope[i] = 0.0;
    for (int i = 0; i + 1 < nk; ++i) {
        const double s = (film[i + 1] - film[i]) / (rise[i + 1] - rise[i]);
        const double at_left = film[i] + s * (2 * rise[i] - rise[i]), at_right = film[i] + s * (2 * rise[i + 1] - rise[i]);
        if (!std::isfinite(s) || !(at_left > 0.0) || !(at_right > 0.0)) {
            set_error("invalid argument: the film curve of mesh %d falls too fast on segment %d (%g K to %g K): the loss density "
                      "h(theta) theta must increase strictly", m, i, rise[i], rise[i + 1]);
            return PADNE_E_INVALID;
        }
        slope[i] = s;
    }
    return PADNE_OK;
}

// the diagonal and hM of the create call back in place, what was derived from A's values dropped
static int film_restore(padne_ctx *ctx, padne_thermal *th) {
    padne_film *fm = th->film;
    csr_invalidate_values(th->A);
    if (th->n_vert > 0) {
        hipLaunchKernelGGL(film_restore_kernel, dim3(nblk(th->n_vert)), dim3(256), 0, ctx->stream, th->n_vert, (const int *)fm->diag,
                           (const double *)fm->D0, th->A->vals);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(th->hM, fm->hM0, sizeof(double) * (size_t)th->n_vert, hipMemcpyDeviceToDevice, ctx->stream));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

// One pass of film_terms_kernel and, with an increment or a count asked for, its fold.  theta: device, [n_vert] at least, or
// null for zeros.  write_matrix: the stored diagonals and fm->c.  increment_out / vertex_out (both or neither): against
// fm->lin.  Synchronises
static int film_pass(padne_ctx *ctx, padne_thermal *th, const double *theta, double *g_out, double *c_out, double *hM_out,
                     bool write_matrix, double *increment_out, int64_t *vertex_out, int64_t *beyond_out) {
    padne_film *fm = th->film;
    hipStream_t s = ctx->stream;
    if (increment_out != nullptr) {
        *increment_out = 0.0;
        *vertex_out = -1;
    }
    if (beyond_out != nullptr) *beyond_out = 0;
    if (th->n_vert == 0) return PADNE_OK;
    const std::vector<long long> vtile = thermal_tiles(th->voff);
    const long long n_vb = vtile[(size_t)th->n_mesh];
    PADNE_REQUIRE(n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const bool inc = increment_out != nullptr, count = inc || beyond_out != nullptr;
    const ErrorMesh M = error_mesh_of(th->L);
    Scratch sc(ctx);
    long long *d_vtile = nullptr, *d_tvert = nullptr, *d_tbeyond = nullptr, *d_out = nullptr;
    double *d_tinc = nullptr, *d_inc = nullptr;
    PADNE_TRY(sc.alloc(&d_vtile, (size_t)th->n_mesh + 1));
    if (count) {
        PADNE_TRY(sc.alloc(&d_tbeyond, (size_t)n_vb));
        PADNE_TRY(sc.alloc(&d_out, 2));
        PADNE_TRY(sc.alloc(&d_inc, 1));
    }
    if (inc) {
        PADNE_TRY(sc.alloc(&d_tinc, (size_t)n_vb));
        PADNE_TRY(sc.alloc(&d_tvert, (size_t)n_vb));
    }
    PADNE_HIP_CHECK(hipMemcpyAsync(d_vtile, vtile.data(), sizeof(long long) * ((size_t)th->n_mesh + 1), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(film_terms_kernel, dim3((unsigned)n_vb), dim3(256), 0, s, th->n_mesh, (const long long *)d_vtile, M.voff,
                       (const int *)fm->kptr, (const double *)fm->krise, (const double *)fm->kfilm, (const double *)fm->kslope,
                       (const double *)th->Mv, theta, (const double *)fm->lin, g_out, write_matrix ? fm->c : c_out, hM_out,
                       (const int *)fm->diag, (const double *)fm->D0, (const double *)fm->hM0,
                       write_matrix ? th->A->vals : (double *)nullptr, d_tinc, d_tvert, d_tbeyond);
    PADNE_HIP_CHECK(hipGetLastError());
    double h_inc = 0.0;
    long long h_out[2] = {kErrNoFace, 0};
    if (count) {
        hipLaunchKernelGGL(film_fold_kernel, dim3(1), dim3(256), 0, s, n_vb, (const double *)d_tinc, (const long long *)d_tvert,
                           (const long long *)d_tbeyond, d_inc, d_out, d_out + 1);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, s));
        if (inc) PADNE_HIP_CHECK(hipMemcpyAsync(&h_inc, d_inc, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));           // (also: the tile table has been read)
    if (inc) {
        *increment_out = h_inc;
        *vertex_out = h_out[0] == kErrNoFace ? -1 : h_out[0];
    }
    if (beyond_out != nullptr) *beyond_out = h_out[1];
    return PADNE_OK;
}

static int film_require(const char *entry, padne_ctx *ctx, const padne_thermal *th) {
    PADNE_TRY(thermal_require(entry, ctx, th));
    PADNE_REQUIRE(th->film != nullptr, (std::string(entry) + ": the handle has no film curves (padne_thermal_set_film_curves)").c_str());
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_thermal_set_film_curves(padne_ctx *ctx, padne_thermal *th, int32_t n_mesh, const int32_t *knot_ptr,
                                             const double *knot_rise, const double *knot_film) {
    PADNE_TRY(thermal_require("padne_thermal_set_film_curves", ctx, th));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (n_mesh == 0) {                                  // the curves go, the handle is the create call's again
        if (th->film == nullptr) return PADNE_OK;
        PADNE_TRY(film_restore(ctx, th));
        film_free(ctx, th->film);
        th->film = nullptr;
        th->solved = false;
        return PADNE_OK;
    }
    PADNE_REQUIRE(n_mesh == th->n_mesh, "n_mesh must be that of the system's mesh, or 0 to remove the curves");
    PADNE_REQUIRE(knot_ptr && knot_rise && knot_film, "null argument");
    PADNE_REQUIRE(knot_ptr[0] == 0, "knot_ptr starts at 0");
    for (int m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(knot_ptr[m + 1] > knot_ptr[m] && knot_ptr[m + 1] - knot_ptr[m] <= kFilmKnots, "between 1 and 64 knots per mesh");
    const int n_knot = knot_ptr[n_mesh];
    std::vector<double> slope((size_t)n_knot);
    for (int m = 0; m < n_mesh; ++m) {
        const int k0 = knot_ptr[m];
        PADNE_TRY(film_check_table(m, knot_ptr[m + 1] - k0, knot_rise + k0, knot_film + k0, slope.data() + k0));
        if (std::memcmp(&knot_film[k0], &th->film_host[(size_t)m], sizeof(double)) != 0) {
            set_error("invalid argument: the film curve of mesh %d starts at %.17g, the handle was created with the film %.17g", m,
                      knot_film[k0], th->film_host[(size_t)m]);
            return PADNE_E_INVALID;
        }
    }
    PADNE_REQUIRE(th->A->nnz <= 0x7fffffffLL, "too many entries");
    if (th->film != nullptr) {                          // new curves replace the old ones
        PADNE_TRY(film_restore(ctx, th));
        film_free(ctx, th->film);
        th->film = nullptr;
    }
    padne_film *fm = new padne_film;
    struct Guard {
        padne_ctx *ctx;
        padne_film *fm;
        ~Guard() { film_free(ctx, fm); }
    } guard{ctx, fm};
    fm->knot_ptr.assign(knot_ptr, knot_ptr + n_mesh + 1);
    fm->rise.assign(knot_rise, knot_rise + n_knot);
    fm->film.assign(knot_film, knot_film + n_knot);
    const size_t nv = (size_t)(th->n_vert > 0 ? th->n_vert : 1), np = (size_t)(th->n_pot > 0 ? th->n_pot : 1);
    fm->kptr = (int *)pool_alloc(ctx, sizeof(int) * ((size_t)n_mesh + 1));
    fm->krise = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_knot);
    fm->kfilm = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_knot);
    fm->kslope = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_knot);
    fm->diag = (int *)pool_alloc(ctx, sizeof(int) * nv);
    fm->D0 = (double *)pool_alloc(ctx, sizeof(double) * nv);
    fm->hM0 = (double *)pool_alloc(ctx, sizeof(double) * nv);
    fm->c = (double *)pool_alloc(ctx, sizeof(double) * nv);
    fm->lin = (double *)pool_alloc(ctx, sizeof(double) * np);
    fm->b0 = (double *)pool_alloc(ctx, sizeof(double) * np);
    if (!fm->kptr || !fm->krise || !fm->kfilm || !fm->kslope || !fm->diag || !fm->D0 || !fm->hM0 || !fm->c || !fm->lin || !fm->b0)
        return PADNE_E_NOMEM;
    Scratch sc(ctx);
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    PADNE_HIP_CHECK(hipMemcpyAsync(fm->kptr, knot_ptr, sizeof(int) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(fm->krise, knot_rise, sizeof(double) * (size_t)n_knot, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(fm->kfilm, knot_film, sizeof(double) * (size_t)n_knot, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(fm->kslope, slope.data(), sizeof(double) * (size_t)n_knot, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemsetAsync(fm->c, 0, sizeof(double) * nv, s));
    PADNE_HIP_CHECK(hipMemsetAsync(fm->lin, 0, sizeof(double) * np, s));
    if (th->n_vert > 0) {
        hipLaunchKernelGGL(film_diag_kernel, dim3(nblk(th->n_vert)), dim3(256), 0, s, th->n_vert, (const int32_t *)th->A->rowptr,
                           (const int32_t *)th->A->cols, (const double *)th->A->vals, fm->diag, fm->D0, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(fm->hM0, th->hM, sizeof(double) * (size_t)th->n_vert, hipMemcpyDeviceToDevice, s));
    }
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));           // (also: the host tables have been read)
    PADNE_REQUIRE(!h_bad, "a vertex row of the thermal matrix has no diagonal");
    guard.fm = nullptr;
    th->film = fm;
    th->solved = false;
    return PADNE_OK;
}

extern "C" int padne_thermal_film_terms(padne_ctx *ctx, padne_thermal *th, const double *theta_host, double *g_out, double *c_out,
                                        double *hM_out, int64_t *beyond_out) {
    PADNE_TRY(film_require("padne_thermal_film_terms", ctx, th));
    PADNE_REQUIRE(beyond_out != nullptr, "null argument");
    *beyond_out = 0;
    if (th->n_vert == 0) return PADNE_OK;
    PADNE_REQUIRE(theta_host && g_out && c_out && hM_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t bytes = sizeof(double) * (size_t)th->n_vert;
    Scratch sc(ctx);
    double *d_theta = nullptr, *d_g = nullptr, *d_c = nullptr, *d_hM = nullptr;
    PADNE_TRY(sc.alloc(&d_theta, (size_t)th->n_vert));
    PADNE_TRY(sc.alloc(&d_g, (size_t)th->n_vert));
    PADNE_TRY(sc.alloc(&d_c, (size_t)th->n_vert));
    PADNE_TRY(sc.alloc(&d_hM, (size_t)th->n_vert));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_theta, theta_host, bytes, hipMemcpyHostToDevice, s));
    PADNE_TRY(film_pass(ctx, th, d_theta, d_g, d_c, d_hM, false, nullptr, nullptr, beyond_out));
    PADNE_HIP_CHECK(hipMemcpyAsync(g_out, d_g, bytes, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(c_out, d_c, bytes, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(hM_out, d_hM, bytes, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_thermal_film_linearise(padne_ctx *ctx, padne_thermal *th, int32_t from_held) {
    PADNE_TRY(film_require("padne_thermal_film_linearise", ctx, th));
    PADNE_REQUIRE(from_held == 0 || from_held == 1, "from_held is 0 (about zero) or 1 (about the held theta)");
    PADNE_REQUIRE(!from_held || (th->solved && th->n_cols == 1), "padne_thermal_film_linearise about the held theta follows a solve of one column");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    padne_film *fm = th->film;
    const size_t np = (size_t)(th->n_pot > 0 ? th->n_pot : 1);
    if (from_held) PADNE_HIP_CHECK(hipMemcpyAsync(fm->lin, th->theta, sizeof(double) * (size_t)th->n_pot, hipMemcpyDeviceToDevice, ctx->stream));
    else PADNE_HIP_CHECK(hipMemsetAsync(fm->lin, 0, sizeof(double) * np, ctx->stream));
    fm->warm = from_held != 0;
    csr_invalidate_values(th->A);                       // the hierarchy is rebuilt per round
    return film_pass(ctx, th, from_held ? fm->lin : (const double *)nullptr, nullptr, nullptr, nullptr, true, nullptr, nullptr, nullptr);
}

extern "C" int padne_thermal_film_increment(padne_ctx *ctx, padne_thermal *th, double *increment_out, int64_t *vertex_out,
                                            int64_t *beyond_out) {
    PADNE_TRY(film_require("padne_thermal_film_increment", ctx, th));
    PADNE_REQUIRE(increment_out && vertex_out && beyond_out, "null argument");
    PADNE_REQUIRE(th->solved && th->n_cols == 1, "padne_thermal_film_increment follows a solve of one column");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    return film_pass(ctx, th, th->theta, nullptr, nullptr, th->hM, false, increment_out, vertex_out, beyond_out);
}

extern "C" int padne_thermal_resolve(padne_ctx *ctx, padne_thermal *th, const padne_solve_opts *opts, double *theta_host,
                                     padne_solve_info *info) {
    PADNE_TRY(film_require("padne_thermal_resolve", ctx, th));
    PADNE_REQUIRE(th->film->have_load, "padne_thermal_resolve follows a solve on this handle: it holds no load yet");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    return thermal_solve_core(ctx, th, 1, 0, nullptr, nullptr, nullptr, opts, theta_host, info, true);
}

extern "C" int padne_thermal_solve_kkt_column(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols, int32_t col,
                                              int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col,
                                              const double *heat_val, const padne_solve_opts *opts, double *theta_host,
                                              padne_solve_info *info) {
    const double *V = nullptr;
    PADNE_TRY(thermal_kkt_block("padne_thermal_solve_kkt_column", ctx, th, plan, n_cols, &V));
    PADNE_REQUIRE(col >= 0 && col < n_cols, "the column must be one of the finished block's");
    PADNE_TRY(thermal_check_heat(th, 1, n_heat, heat_node, heat_col, heat_val));
    PADNE_TRY(thermal_kkt_face_power_column(ctx, th, n_cols, col, V, nullptr));
    return thermal_solve_core(ctx, th, 1, n_heat, heat_node, heat_col, heat_val, opts, theta_host, info);
}
