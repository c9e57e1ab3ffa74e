// Transient electro-thermal: the coupling handle (coupled.hip) and the transient handle (transient.hip) joined, so that the
// resistivity follows the temperature over time ("Transient electro-thermal").  No reference counterpart.
//
// One step from t_n while case j is on, every expression rounded as the kernels it names state it:
//
//     1. mean_f, s_f and d = max_f |mean_f - previous mean_f| from theta_n      padne_coupled_update_transient (here)
//     2. L = L0 + sum_f (s_f - 1) sigma_m K_f                                   padne_coupled_revalue
//     3. the one-column electrical solve of case j on that L                    a padne_kkt plan of the caller
//     4. B[j] = the load of that solve with sigma_m s_f in the face powers      padne_coupled_transient_load (here)
//     5. S theta_{n+1} = (Cv / dt) theta_n + B[j]                               padne_transient_run, one step
//
// Part 1 is coupled_scale_kernel and its fold on the transient handle's state: nothing crosses to the host but the increment.
// Part 4 is the launch sequence of padne_coupled_solve_kkt up to the solve, written into a slot of the load table; behind it
// the heat of every mesh's copper is summed from the same face powers, per tile of 256 faces of one mesh and then by one
// workgroup per mesh, in the order of padne_thermal_report's sums.  The range of the used scale is a minimum and a maximum per
// 256 faces and then one workgroup over the tiles.
//
// Kernels: streams bound by memory, workgroups of 256, no floating-point atomics, the folds in the wave order of error.hpp.
// Bytes moved: the heat tiles read P once (8 per face) and write 8 per tile; the range reads s_used once (8 per face) and
// writes 16 per tile; the folds read what the tiles wrote.  Compiled with -ffp-contract=off: two calls give the same bits.
#include "thermal.hpp"

#include <cmath>
#include <vector>

namespace padne {

// tile_P[b] = the sum of P[t] over the 256 faces of tile b of one mesh (the layout and the order of
// thermal_report_face_kernel)
__global__ __launch_bounds__(256) void coupled_transient_heat_kernel(const int n_mesh, const long long *__restrict__ tile_off,
                                                                     const long long *__restrict__ toff,
                                                                     const double *__restrict__ P, double *__restrict__ tile_P) {
    __shared__ double red[4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    double p = t < toff[m + 1] ? P[t] : 0.0;
    p = error_wave_sum(p);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) tile_P[b] = error_sum4(red);
}

// out[m] = the sum of mesh m's tiles, by one workgroup per mesh in the order of thermal_fold_kernel
__global__ __launch_bounds__(256) void coupled_transient_heat_fold_kernel(const long long *__restrict__ tile_off,
                                                                          const double *__restrict__ tile_P,
                                                                          double *__restrict__ out) {
    __shared__ double red[4];
    const int m = blockIdx.x;
    double s = 0.0;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) s += tile_P[i];
    s = error_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[m] = error_sum4(red);
}

__device__ __forceinline__ void coupled_transient_wave_range(double &lo, double &hi) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ol = __shfl_down(lo, off, 64), oh = __shfl_down(hi, off, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
}

// the workgroup's (lo, hi) at thread 0, from each thread's; red_lo and red_hi: 4 entries of shared memory each
__device__ __forceinline__ void coupled_transient_block_range(double &lo, double &hi, double *red_lo, double *red_hi) {
    coupled_transient_wave_range(lo, hi);
    if ((threadIdx.x & 63) == 0) {
        red_lo[threadIdx.x >> 6] = lo;
        red_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < 4; ++q) {
            lo = red_lo[q] < lo ? red_lo[q] : lo;
            hi = red_hi[q] > hi ? red_hi[q] : hi;
        }
}

// tile_lo[b], tile_hi[b] = the smallest and the largest s[t] of the 256 faces of tile b (+infinity and -infinity past the end)
__global__ __launch_bounds__(256) void coupled_transient_range_kernel(const long long n_tri, const double *__restrict__ s,
                                                                      double *__restrict__ tile_lo, double *__restrict__ tile_hi) {
    __shared__ double red_lo[4], red_hi[4];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    double lo = INFINITY, hi = -INFINITY;
    if (t < n_tri) lo = hi = s[t];
    coupled_transient_block_range(lo, hi, red_lo, red_hi);
    if (threadIdx.x == 0) {
        tile_lo[blockIdx.x] = lo;
        tile_hi[blockIdx.x] = hi;
    }
}

// out[0], out[1] = the smallest tile_lo and the largest tile_hi, by one workgroup
__global__ __launch_bounds__(256) void coupled_transient_range_fold_kernel(const long long n_tiles, const double *__restrict__ tile_lo,
                                                                           const double *__restrict__ tile_hi,
                                                                           double *__restrict__ out) {
    __shared__ double red_lo[4], red_hi[4];
    double lo = INFINITY, hi = -INFINITY;
    for (long long i = threadIdx.x; i < n_tiles; i += 256) {
        lo = tile_lo[i] < lo ? tile_lo[i] : lo;
        hi = tile_hi[i] > hi ? tile_hi[i] : hi;
    }
    coupled_transient_block_range(lo, hi, red_lo, red_hi);
    if (threadIdx.x == 0) {
        out[0] = lo;
        out[1] = hi;
    }
}

// the two handles are the context's and stand on one thermal handle
static int coupled_transient_require(const char *entry, padne_ctx *ctx, const padne_coupled *cp, const padne_transient *tr) {
    PADNE_REQUIRE(ctx && cp && tr, "null argument");
    PADNE_REQUIRE(cp->ctx == ctx && tr->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    PADNE_REQUIRE(cp->th == tr->th, (std::string(entry) + ": the coupling and the transient handle must stand on one thermal handle").c_str());
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_transient_reserve_loads(padne_ctx *ctx, padne_transient *tr, int32_t n_case) {
    PADNE_REQUIRE(ctx && tr, "null argument");
    PADNE_REQUIRE(tr->ctx == ctx, "padne_transient_reserve_loads: the handle belongs to another context");
    PADNE_REQUIRE(n_case >= 1 && n_case <= 4096, "between 1 and 4096 cases");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t count = (size_t)n_case * (size_t)(tr->n_pot > 0 ? tr->n_pot : 1);
    double *B = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (B == nullptr) return PADNE_E_NOMEM;             // (the handle keeps its table)
    if (hipMemsetAsync(B, 0, sizeof(double) * count, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pool_free(ctx, B);
        set_error("padne_transient_reserve_loads: the table could not be cleared");
        return PADNE_E_HIP;
    }
    if (tr->B != nullptr) pool_free(ctx, tr->B);
    tr->B = B;
    tr->n_case = n_case;
    tr->started = false;                                // a running schedule names cases of the old table
    tr->trial_live = false;
    return PADNE_OK;
}

extern "C" int padne_coupled_transient_load(padne_ctx *ctx, padne_coupled *cp, padne_transient *tr, padne_kkt *plan, int32_t slot,
                                            int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col,
                                            const double *heat_val, int32_t n_mesh, double *mesh_heat_out) {
    PADNE_TRY(coupled_transient_require("padne_coupled_transient_load", ctx, cp, tr));
    PADNE_REQUIRE(tr->B != nullptr && tr->n_case >= 1, "padne_coupled_transient_load follows padne_transient_reserve_loads or padne_transient_loads");
    PADNE_REQUIRE(slot >= 0 && slot < tr->n_case, "load slot out of range");
    PADNE_REQUIRE(n_mesh == tr->n_mesh && mesh_heat_out != nullptr, "mesh_heat_out has one entry per mesh");
    padne_thermal *th = tr->th;
    const double *V = nullptr;
    PADNE_TRY(thermal_kkt_block("padne_coupled_transient_load", ctx, th, plan, 1, &V));
    PADNE_TRY(thermal_check_heat(th, 1, n_heat, heat_node, heat_col, heat_val));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const std::vector<long long> ftile = thermal_tiles(th->toff);
    const long long n_fb = ftile[(size_t)n_mesh];
    PADNE_REQUIRE(n_fb <= 0x7fffffffLL, "too many tiles for one launch");
    Scratch sc(ctx);
    double *d_b = nullptr, *d_tP = nullptr, *d_heat = nullptr;
    long long *d_ftile = nullptr;
    PADNE_TRY(sc.alloc(&d_b, (size_t)tr->n_pot));
    PADNE_TRY(sc.alloc(&d_tP, (size_t)n_fb));
    PADNE_TRY(sc.alloc(&d_heat, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_ftile, (size_t)n_mesh + 1));
    // the load of padne_coupled_solve_kkt: the face powers with the used scale, the gather, the triples, the sources -- into
    // scratch, so that a refusal on the way leaves the table as it was
    PADNE_TRY(thermal_kkt_face_power(ctx, th, 1, V, cp->s_used));
    PADNE_TRY(thermal_form_load(ctx, th, 1, n_heat, heat_node, heat_col, heat_val, d_b));
    if (tr->n_pot > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(tr->B + (size_t)slot * (size_t)tr->n_pot, d_b, sizeof(double) * (size_t)tr->n_pot,
                                       hipMemcpyDeviceToDevice, st));
    // (pageable host memory: the copy is staged before the call returns, so the table may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ftile, ftile.data(), sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, st));
    if (n_fb > 0) {
        hipLaunchKernelGGL(coupled_transient_heat_kernel, dim3((unsigned)n_fb), dim3(256), 0, st, (int)n_mesh,
                           (const long long *)d_ftile, error_mesh_of(th->L).toff, (const double *)th->P, d_tP);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(coupled_transient_heat_fold_kernel, dim3((unsigned)n_mesh), dim3(256), 0, st, (const long long *)d_ftile,
                       (const double *)d_tP, d_heat);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_heat_out, d_heat, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    return PADNE_OK;
}

extern "C" int padne_coupled_update_transient(padne_ctx *ctx, padne_coupled *cp, const padne_transient *tr, int32_t col,
                                              double *increment_out) {
    PADNE_TRY(coupled_transient_require("padne_coupled_update_transient", ctx, cp, tr));
    PADNE_REQUIRE(increment_out != nullptr, "null argument");
    PADNE_REQUIRE(tr->started && tr->theta != nullptr, "padne_coupled_update_transient follows padne_transient_start");
    PADNE_REQUIRE(col >= 0 && col < tr->n_cols, "column out of range");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    return coupled_run_scale(ctx, cp, tr->theta + (size_t)col * (size_t)tr->n_pot, increment_out);
}

extern "C" int padne_coupled_scale_range(padne_ctx *ctx, const padne_coupled *cp, double *min_out, double *max_out) {
    PADNE_REQUIRE(ctx && cp && min_out && max_out, "null argument");
    PADNE_REQUIRE(cp->ctx == ctx, "padne_coupled_scale_range: the handle belongs to another context");
    PADNE_REQUIRE(cp->n_tri > 0, "the system's mesh has no face");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long n_tiles = nblk(cp->n_tri);
    Scratch sc(ctx);
    double *d_lo = nullptr, *d_hi = nullptr, *d_out = nullptr;
    PADNE_TRY(sc.alloc(&d_lo, (size_t)n_tiles));
    PADNE_TRY(sc.alloc(&d_hi, (size_t)n_tiles));
    PADNE_TRY(sc.alloc(&d_out, 2));
    hipLaunchKernelGGL(coupled_transient_range_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, cp->n_tri,
                       (const double *)cp->s_used, d_lo, d_hi);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(coupled_transient_range_fold_kernel, dim3(1), dim3(256), 0, st, n_tiles, (const double *)d_lo,
                       (const double *)d_hi, d_out);
    PADNE_HIP_CHECK(hipGetLastError());
    double h_out[2] = {0.0, 0.0};
    PADNE_HIP_CHECK(hipMemcpyAsync(h_out, d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    *min_out = h_out[0];
    *max_out = h_out[1];
    return PADNE_OK;
}
