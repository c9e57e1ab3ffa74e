// The periodic steady state of a duty cycle: the Krylov arithmetic on the transient handle's columns ("Periodic
// steady state").  No reference counterpart.
//
// The period map of the fixed-step scheme of transient.hip is affine, theta(T) = Phi theta(0) + d, so the periodic state solves
// (I - Phi) theta* = d.  The host runs GMRES without restart on it, per column, all columns in lockstep; a product with
// I - Phi is one period of padne_transient_run with the sources off.  This file holds what that needs on the device: a state
// put into the transient handle, and the inner products, updates and combinations of the basis, which never leaves the
// device.  <x, y>_C = sum_v Cv[v] x[v] y[v] over the vertices: Phi is self-adjoint in it, and Cv is on the transient handle.
//
//     mark:      x0 = state
//     residual:  r0 = state - x0;  beta[c] = sqrt(<r0, r0>_C);  v_0 = r0 / beta (zeros where beta is not positive)
//     load j:    state = v_j
//     push j:    w = v_j - state
//                twice:  d_i = <w, v_i>_C for i = 0 .. j;   w -= sum_i d_i v_i          (classical Gram-Schmidt, twice)
//                h_i = d_i(first) + d_i(second);  h_{j+1} = sqrt(<w, w>_C);  v_{j+1} = w / h_{j+1} (zeros where not positive)
//     predict:   max_v |r0 - sum_i coef_i v_i|
//     combine:   state = x0 + sum_i y_i v_i
//
// Vectors carry all n_pot entries (the internal nodes ride along linearly: they only ever serve as guesses of a step's
// solve); dots, norms and tops run over the vertices.  Every expression rounds as written (-ffp-contract=off):
//
//     dot:     term[v] = (Cv[v] * w[v]) * V_i[v]; tiles of 256 vertices of the column's whole vertex range by the order of
//              error.hpp, the tiles folded by one workgroup whose thread t takes tiles t, t + 256, ... front to back
//     update:  s = 0.0; s = s + d_i * V_i[e] for i ascending; w[e] = w[e] - s
//     combine: a = base[e]; a = a + c_i * V_i[e] for i ascending
//     top:     the largest |a| over the vertices with the lowest vertex on a tie, by the same tiles and fold; a value that is
//              not finite counts as +infinity (sdirk.hip)
//
// All kernels are streams bound by memory, one lane per entry and column (grid y: every column goes through one launch).  A
// dot launch reads w once and up to 8 basis vectors, so a lane has up to 10 independent 8-byte loads in flight, a wave 5 KB;
// the update and the combination loop over the basis in one launch, which the compiler unrolls to the same effect.  Per
// column the dots of a Gram-Schmidt pass move (j + 2) n 8 bytes (w per chunk of 8 on top), the update (j + 3) n 8, the
// combination (j + 2) n 8.  No floating-point atomics: two calls give the same bits.
#include "thermal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

struct padne_periodic {
    padne_ctx *ctx = nullptr;
    padne_transient *tr = nullptr;           // borrowed
    long long n_pot = 0, n_vert = 0;
    int n_cols = 0, max_vectors = 0;
    double *x0 = nullptr, *r0 = nullptr, *w = nullptr;      // [n_cols][n_pot]
    double *V = nullptr;                     // [max_vectors][n_cols][n_pot]
    bool marked = false, have_r0 = false;
    int n_vec = 0;                           // basis vectors that hold something
};

namespace padne {

constexpr int kPeriodicChunk = 8;            // basis vectors per pass over w
constexpr int kPeriodicSlots = kPeriodicChunk + 1;       // + the norm

// out[c][e] = a[c][e] - b[c][e]; c = blockIdx.y
__global__ __launch_bounds__(256) void periodic_diff_kernel(const long long n_pot, const double *__restrict__ a,
                                                            const double *__restrict__ b, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pot) return;
    const long long at = (long long)blockIdx.y * n_pot + e;
    out[at] = a[at] - b[at];
}

// Per tile b = blockIdx.x of 256 vertices and column c = blockIdx.y: part[c][s][b] = the tile's sum of (Cv w) V_{first + s}
// for s < n (n <= 8), and with `norm` part[c][8][b] = that of (Cv w) w.  w is read once
__global__ __launch_bounds__(256) void periodic_dot_kernel(const long long n_pot, const long long n_vert, const long long n_tiles,
                                                           const int n_cols, const double *__restrict__ Cv,
                                                           const double *__restrict__ w, const double *__restrict__ V,
                                                           const int first, const int n, const int norm,
                                                           double *__restrict__ part) {
    __shared__ double red[kPeriodicSlots][4];
    const long long b = blockIdx.x, c = blockIdx.y;
    const long long v = b * 256 + threadIdx.x;
    double acc[kPeriodicSlots];
#pragma unroll
    for (int s = 0; s < kPeriodicSlots; ++s) acc[s] = 0.0;
    if (v < n_vert) {
        const double wv = w[c * n_pot + v];
        const double cw = Cv[v] * wv;
#pragma unroll
        for (int s = 0; s < kPeriodicChunk; ++s)
            if (s < n) acc[s] = cw * V[((long long)(first + s) * n_cols + c) * n_pot + v];
        if (norm) acc[kPeriodicChunk] = cw * wv;
    }
#pragma unroll
    for (int s = 0; s < kPeriodicSlots; ++s) {
        if (s < kPeriodicChunk ? s < n : norm != 0) {
            const double t = error_wave_sum(acc[s]);
            if ((threadIdx.x & 63) == 0) red[s][threadIdx.x >> 6] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x < kPeriodicSlots) {
        const int s = threadIdx.x;
        if (s < kPeriodicChunk ? s < n : norm != 0) part[(c * kPeriodicSlots + s) * n_tiles + b] = error_sum4(red[s]);
    }
}

// Per slot s = blockIdx.x and column c = blockIdx.y, the fold of the column's tiles: dots[c][first + s] for s < n (row length
// ld), nrm[c] for the norm's slot
__global__ __launch_bounds__(256) void periodic_fold_kernel(const long long n_tiles, const int first, const int n, const int norm,
                                                            const int ld, const double *__restrict__ part,
                                                            double *__restrict__ dots, double *__restrict__ nrm) {
    __shared__ double red[4];
    const int s = blockIdx.x;
    if (!(s < kPeriodicChunk ? s < n : norm != 0)) return;
    const long long c = blockIdx.y;
    const double *p = part + (c * kPeriodicSlots + s) * n_tiles;
    double a = 0.0;
    for (long long i = threadIdx.x; i < n_tiles; i += 256) a += p[i];
    a = error_wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double total = error_sum4(red);
        if (s < kPeriodicChunk) dots[c * ld + first + s] = total;
        else nrm[c] = total;
    }
}

// w[c][e] -= sum_{i < n} d[c][i] V_i[c][e], the sum from 0.0 in ascending i
__global__ __launch_bounds__(256) void periodic_update_kernel(const long long n_pot, const int n_cols, const int n, const int ld,
                                                              const double *__restrict__ d, const double *__restrict__ V,
                                                              double *__restrict__ w) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pot) return;
    const long long c = blockIdx.y;
    const long long at = c * n_pot + e;
    const long long stride = (long long)n_cols * n_pot;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + d[c * ld + i] * V[i * stride + at];
    w[at] = w[at] - s;
}

// out[c][e] = w[c][e] / h[c] where h[c] is positive, 0.0 elsewhere (a frozen column)
__global__ __launch_bounds__(256) void periodic_scale_kernel(const long long n_pot, const double *__restrict__ h,
                                                             const double *__restrict__ w, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pot) return;
    const long long at = (long long)blockIdx.y * n_pot + e;
    const double hc = h[blockIdx.y];
    out[at] = hc > 0.0 ? w[at] / hc : 0.0;
}

__device__ __forceinline__ double periodic_combination(const long long at, const long long stride, const long long c, const int n,
                                                       const int ld, const double *__restrict__ base,
                                                       const double *__restrict__ coef, const double *__restrict__ V) {
    double a = base[at];
    for (int i = 0; i < n; ++i) a = a + coef[c * ld + i] * V[i * stride + at];
    return a;
}

// out[c][e] = base[c][e] + sum_{i < n} coef[c][i] V_i[c][e] over all n_pot entries
__global__ __launch_bounds__(256) void periodic_combine_kernel(const long long n_pot, const int n_cols, const int n, const int ld,
                                                               const double *__restrict__ base, const double *__restrict__ coef,
                                                               const double *__restrict__ V, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pot) return;
    const long long c = blockIdx.y;
    const long long at = c * n_pot + e;
    out[at] = periodic_combination(at, (long long)n_cols * n_pot, c, n, ld, base, coef, V);
}

// Per tile b = blockIdx.x of 256 vertices and column c = blockIdx.y: the largest |combination| and its vertex at [c][b];
// nothing is written but the tops
__global__ __launch_bounds__(256) void periodic_top_kernel(const long long n_pot, const long long n_vert, const long long n_tiles,
                                                           const int n_cols, const int n, const int ld,
                                                           const double *__restrict__ base, const double *__restrict__ coef,
                                                           const double *__restrict__ V, double *__restrict__ tile_max,
                                                           long long *__restrict__ tile_vert) {
    __shared__ double red_v[4];
    __shared__ long long red_f[4];
    const long long b = blockIdx.x, c = blockIdx.y;
    const long long v = b * 256 + threadIdx.x;
    double a = -INFINITY;
    long long f = kErrNoFace;
    if (v < n_vert) {
        a = fabs(periodic_combination(c * n_pot + v, (long long)n_cols * n_pot, c, n, ld, base, coef, V));
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
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        tile_max[c * n_tiles + b] = a;
        tile_vert[c * n_tiles + b] = f;
    }
}

// Per column c = blockIdx.x, over its tiles: the largest tile top and its vertex (-infinity and -1 without vertices)
__global__ __launch_bounds__(256) void periodic_fold_top_kernel(const long long n_tiles, const double *__restrict__ tile_v,
                                                                const long long *__restrict__ tile_f, double *__restrict__ out_v,
                                                                long long *__restrict__ out_f) {
    __shared__ double red_v[4];
    __shared__ long long red_f[4];
    const long long at = (long long)blockIdx.x * n_tiles;
    double a = -INFINITY;
    long long f = kErrNoFace;
    for (long long i = threadIdx.x; i < n_tiles; i += 256) error_merge(a, f, tile_v[at + i], tile_f[at + i]);
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        out_v[blockIdx.x] = a;
        out_f[blockIdx.x] = f == kErrNoFace ? -1 : f;
    }
}

static void periodic_free(padne_periodic *pd) {
    if (pd == nullptr) return;
    padne_ctx *ctx = pd->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)pd->x0, (void *)pd->r0, (void *)pd->w, (void *)pd->V})
        if (p != nullptr) pool_free(ctx, p);
    delete pd;
}

// the handle is the context's and stands on a started transient handle with its number of columns
static int periodic_require(const char *entry, padne_ctx *ctx, const padne_periodic *pd) {
    PADNE_REQUIRE(ctx && pd, "null argument");
    PADNE_REQUIRE(pd->ctx == ctx && pd->tr->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    PADNE_REQUIRE(pd->tr->started && pd->tr->n_cols == pd->n_cols && pd->tr->theta != nullptr,
                  (std::string(entry) + ": the transient handle has been started anew with another number of columns, or not at all").c_str());
    return PADNE_OK;
}

static long long periodic_tiles(const padne_periodic *pd) { return (pd->n_vert + 255) / 256; }
static size_t periodic_count(const padne_periodic *pd) { return (size_t)pd->n_cols * (size_t)pd->n_pot; }
static double *periodic_vector(const padne_periodic *pd, int j) { return pd->V + (size_t)j * periodic_count(pd); }

// the scratch of the dots: tile sums [n_cols][9][n_tiles]
static int periodic_part(padne_periodic *pd, Scratch &sc, double **part) {
    const long long nt = periodic_tiles(pd);
    return sc.alloc(part, (size_t)pd->n_cols * kPeriodicSlots * (size_t)(nt > 0 ? nt : 1));
}

// d[c][i] = <w, v_i>_C for i < n (d: [n_cols][max_vectors] on the device), in chunks of 8; n = 0 with nrm: nrm[c] = <w, w>_C alone
static int periodic_dots(padne_periodic *pd, const double *w, int n, double *part, double *d, double *nrm) {
    hipStream_t s = pd->ctx->stream;
    const long long nt = periodic_tiles(pd);
    PADNE_REQUIRE(nt <= 0x7fffffffLL, "too many tiles for one launch");
    const int norm = n == 0 ? 1 : 0;
    for (int first = 0; first < (norm ? 1 : n); first += kPeriodicChunk) {
        const int m = n - first < kPeriodicChunk ? n - first : kPeriodicChunk;
        if (nt > 0) {
            hipLaunchKernelGGL(periodic_dot_kernel, dim3((unsigned)nt, (unsigned)pd->n_cols), dim3(256), 0, s, pd->n_pot, pd->n_vert, nt,
                               pd->n_cols, (const double *)pd->tr->Cv, w, (const double *)pd->V, first, m, norm, part);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(periodic_fold_kernel, dim3(kPeriodicSlots, (unsigned)pd->n_cols), dim3(256), 0, s, nt, first, m, norm,
                           pd->max_vectors, (const double *)part, d, nrm);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return PADNE_OK;
}

static int periodic_update(padne_periodic *pd, int n, const double *d, double *w) {
    if (pd->n_pot == 0 || n == 0) return PADNE_OK;
    hipLaunchKernelGGL(periodic_update_kernel, dim3(nblk(pd->n_pot), (unsigned)pd->n_cols), dim3(256), 0, pd->ctx->stream, pd->n_pot,
                       pd->n_cols, n, pd->max_vectors, d, (const double *)pd->V, w);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

// out = w / h[c] (h on the host), zeros where h[c] is not positive
static int periodic_scale(padne_periodic *pd, Scratch &sc, const std::vector<double> &h, const double *w, double *out) {
    double *d_h = nullptr;
    PADNE_TRY(sc.alloc(&d_h, h.size()));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_h, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, pd->ctx->stream));
    if (pd->n_pot > 0) {
        hipLaunchKernelGGL(periodic_scale_kernel, dim3(nblk(pd->n_pot), (unsigned)pd->n_cols), dim3(256), 0, pd->ctx->stream, pd->n_pot,
                           (const double *)d_h, w, out);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(pd->ctx->stream));          // (the copy has read h)
    return PADNE_OK;
}

// coef[n_cols][n] of the host, times `sign`, as rows of length max_vectors on the device
static int periodic_upload(padne_periodic *pd, Scratch &sc, int n, const double *coef, double sign, double **d_coef) {
    std::vector<double> rows((size_t)pd->n_cols * (size_t)pd->max_vectors, 0.0);
    for (int c = 0; c < pd->n_cols; ++c)
        for (int i = 0; i < n; ++i) rows[(size_t)c * pd->max_vectors + i] = sign * coef[(size_t)c * n + i];
    PADNE_TRY(sc.alloc(d_coef, rows.size()));
    PADNE_HIP_CHECK(hipMemcpyAsync(*d_coef, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, pd->ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(pd->ctx->stream));
    return PADNE_OK;
}

// max_v |base + sum_i coef_i v_i| per column with its vertex (0.0 and -1 without vertices), on the host
static int periodic_top(padne_periodic *pd, Scratch &sc, const double *base, int n, const double *d_coef, double *max_out,
                        int64_t *vert_out) {
    hipStream_t s = pd->ctx->stream;
    const long long nt = periodic_tiles(pd);
    PADNE_REQUIRE(nt <= 0x7fffffffLL, "too many tiles for one launch");
    const size_t cells = (size_t)pd->n_cols * (size_t)(nt > 0 ? nt : 1);
    double *t_max = nullptr, *d_max = nullptr;
    long long *t_vert = nullptr, *d_vert = nullptr;
    PADNE_TRY(sc.alloc(&t_max, cells));
    PADNE_TRY(sc.alloc(&t_vert, cells));
    PADNE_TRY(sc.alloc(&d_max, (size_t)pd->n_cols));
    PADNE_TRY(sc.alloc(&d_vert, (size_t)pd->n_cols));
    if (nt > 0) {
        hipLaunchKernelGGL(periodic_top_kernel, dim3((unsigned)nt, (unsigned)pd->n_cols), dim3(256), 0, s, pd->n_pot, pd->n_vert, nt,
                           pd->n_cols, n, pd->max_vectors, base, d_coef, (const double *)pd->V, t_max, t_vert);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(periodic_fold_top_kernel, dim3((unsigned)pd->n_cols), dim3(256), 0, s, nt, (const double *)t_max,
                       (const long long *)t_vert, d_max, d_vert);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<long long> h_vert((size_t)pd->n_cols);
    PADNE_HIP_CHECK(hipMemcpyAsync(max_out, d_max, sizeof(double) * (size_t)pd->n_cols, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(h_vert.data(), d_vert, sizeof(long long) * (size_t)pd->n_cols, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < pd->n_cols; ++c) {
        vert_out[c] = h_vert[(size_t)c];
        if (h_vert[(size_t)c] < 0) max_out[c] = 0.0;
    }
    return PADNE_OK;
}

// What padne_transient_start does once the state is in place: no live trial, the clock at 0, the envelope the state with step 0
static int periodic_restart(padne_periodic *pd) {
    padne_transient *tr = pd->tr;
    tr->trial_live = false;
    tr->step = 0;
    tr->time = 0.0;
    Scratch sc(pd->ctx);
    TransientPass ps;
    double *d_res = nullptr;
    long long *d_vert = nullptr;
    const size_t cells = (size_t)tr->n_cols * (size_t)tr->n_mesh;
    PADNE_TRY(transient_pass_init(tr, sc, &ps));
    PADNE_TRY(sc.alloc(&d_res, 3 * cells));
    PADNE_TRY(sc.alloc(&d_vert, cells));
    PADNE_TRY(transient_pass(tr, ps, tr->theta, 1, tr->step, d_res, d_res + cells, d_res + 2 * cells, d_vert));
    PADNE_HIP_CHECK(hipStreamSynchronize(pd->ctx->stream));
    return PADNE_OK;
}

// sqrt of a squared norm: 0.0 stays, anything that is no number is handed on as it is
static double periodic_root(double sq) { return sq > 0.0 ? std::sqrt(sq) : sq; }

}  // namespace padne

using namespace padne;

extern "C" int padne_periodic_create(padne_ctx *ctx, padne_transient *tr, int32_t max_vectors, padne_periodic **out) {
    PADNE_REQUIRE(ctx && tr && out, "null argument");
    PADNE_TRY(transient_require("padne_periodic_create", ctx, tr));
    PADNE_REQUIRE(tr->started && tr->theta != nullptr, "padne_periodic_create follows padne_transient_start");
    PADNE_REQUIRE(max_vectors >= 1 && max_vectors <= 4095, "between 1 and 4095 basis vectors");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    padne_periodic *pd = new padne_periodic;
    pd->ctx = ctx;
    pd->tr = tr;
    pd->n_pot = tr->n_pot;
    pd->n_vert = tr->n_vert;
    pd->n_cols = tr->n_cols;
    pd->max_vectors = max_vectors;
    struct Guard {
        padne_periodic *pd;
        ~Guard() { periodic_free(pd); }
    } guard{pd};
    // (n_cols <= 4096, max_vectors <= 4095 and n_pot < 2^31: the byte count fits 64 bits)
    PADNE_REQUIRE(pd->n_pot <= 0x7fffffffLL, "too many unknowns");
    const size_t count = periodic_count(pd) > 0 ? periodic_count(pd) : 1;
    pd->x0 = (double *)pool_alloc(ctx, sizeof(double) * count);
    pd->r0 = (double *)pool_alloc(ctx, sizeof(double) * count);
    pd->w = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (!pd->x0 || !pd->r0 || !pd->w) return PADNE_E_NOMEM;
    pd->V = (double *)pool_alloc(ctx, sizeof(double) * count * (size_t)max_vectors);
    if (!pd->V) return PADNE_E_NOMEM;
    guard.pd = nullptr;
    *out = pd;
    return PADNE_OK;
}

extern "C" int padne_periodic_destroy(padne_periodic *pd) {
    periodic_free(pd);
    return PADNE_OK;
}

extern "C" int padne_periodic_mark(padne_ctx *ctx, padne_periodic *pd) {
    PADNE_TRY(periodic_require("padne_periodic_mark", ctx, pd));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    if (periodic_count(pd) > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(pd->x0, pd->tr->theta, sizeof(double) * periodic_count(pd), hipMemcpyDeviceToDevice, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    pd->marked = true;
    pd->have_r0 = false;
    pd->n_vec = 0;
    return PADNE_OK;
}

extern "C" int padne_periodic_residual(padne_ctx *ctx, padne_periodic *pd, double *beta_out, double *max_out, int64_t *vertex_out) {
    PADNE_TRY(periodic_require("padne_periodic_residual", ctx, pd));
    PADNE_REQUIRE(pd->marked, "padne_periodic_residual follows padne_periodic_mark");
    PADNE_REQUIRE(beta_out && max_out && vertex_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    double *part = nullptr, *d_nrm = nullptr;
    PADNE_TRY(periodic_part(pd, sc, &part));
    PADNE_TRY(sc.alloc(&d_nrm, (size_t)pd->n_cols));
    if (pd->n_pot > 0) {
        hipLaunchKernelGGL(periodic_diff_kernel, dim3(nblk(pd->n_pot), (unsigned)pd->n_cols), dim3(256), 0, s, pd->n_pot,
                           (const double *)pd->tr->theta, (const double *)pd->x0, pd->r0);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_TRY(periodic_dots(pd, pd->r0, 0, part, nullptr, d_nrm));
    std::vector<double> beta((size_t)pd->n_cols);
    PADNE_HIP_CHECK(hipMemcpyAsync(beta.data(), d_nrm, sizeof(double) * beta.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    for (double &b : beta) b = periodic_root(b);
    PADNE_TRY(periodic_scale(pd, sc, beta, pd->r0, periodic_vector(pd, 0)));
    PADNE_TRY(periodic_top(pd, sc, pd->r0, 0, nullptr, max_out, vertex_out));
    for (int c = 0; c < pd->n_cols; ++c) beta_out[c] = beta[(size_t)c];
    pd->have_r0 = true;
    pd->n_vec = 1;
    return PADNE_OK;
}

extern "C" int padne_periodic_load(padne_ctx *ctx, padne_periodic *pd, int32_t j) {
    PADNE_TRY(periodic_require("padne_periodic_load", ctx, pd));
    PADNE_REQUIRE(j >= 0 && j < pd->n_vec, "no such basis vector yet");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    if (periodic_count(pd) > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(pd->tr->theta, periodic_vector(pd, j), sizeof(double) * periodic_count(pd), hipMemcpyDeviceToDevice,
                                       ctx->stream));
    return periodic_restart(pd);
}

extern "C" int padne_periodic_push(padne_ctx *ctx, padne_periodic *pd, int32_t j, double *h_out) {
    PADNE_TRY(periodic_require("padne_periodic_push", ctx, pd));
    PADNE_REQUIRE(pd->n_vec >= 1 && j == pd->n_vec - 1, "padne_periodic_push takes the newest basis vector");
    PADNE_REQUIRE(j + 1 < pd->max_vectors, "the basis is full");
    PADNE_REQUIRE(h_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = j + 1, ld = pd->max_vectors;
    Scratch sc(ctx);
    double *part = nullptr, *d1 = nullptr, *d2 = nullptr, *d_nrm = nullptr;
    PADNE_TRY(periodic_part(pd, sc, &part));
    PADNE_TRY(sc.alloc(&d1, (size_t)pd->n_cols * ld));
    PADNE_TRY(sc.alloc(&d2, (size_t)pd->n_cols * ld));
    PADNE_TRY(sc.alloc(&d_nrm, (size_t)pd->n_cols));
    if (pd->n_pot > 0) {
        hipLaunchKernelGGL(periodic_diff_kernel, dim3(nblk(pd->n_pot), (unsigned)pd->n_cols), dim3(256), 0, s, pd->n_pot,
                           (const double *)periodic_vector(pd, j), (const double *)pd->tr->theta, pd->w);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    for (double *d : {d1, d2}) {
        PADNE_TRY(periodic_dots(pd, pd->w, n, part, d, nullptr));
        PADNE_TRY(periodic_update(pd, n, d, pd->w));
    }
    PADNE_TRY(periodic_dots(pd, pd->w, 0, part, nullptr, d_nrm));
    std::vector<double> h1((size_t)pd->n_cols * ld), h2((size_t)pd->n_cols * ld), next((size_t)pd->n_cols);
    PADNE_HIP_CHECK(hipMemcpyAsync(h1.data(), d1, sizeof(double) * h1.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(h2.data(), d2, sizeof(double) * h2.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(next.data(), d_nrm, sizeof(double) * next.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    for (double &x : next) x = periodic_root(x);
    PADNE_TRY(periodic_scale(pd, sc, next, pd->w, periodic_vector(pd, j + 1)));
    for (int c = 0; c < pd->n_cols; ++c) {
        for (int i = 0; i < n; ++i) h_out[(size_t)c * (n + 1) + i] = h1[(size_t)c * ld + i] + h2[(size_t)c * ld + i];
        h_out[(size_t)c * (n + 1) + n] = next[(size_t)c];
    }
    pd->n_vec = j + 2;
    return PADNE_OK;
}

extern "C" int padne_periodic_predict(padne_ctx *ctx, padne_periodic *pd, int32_t n_coef, const double *coef, double *max_out,
                                      int64_t *vertex_out) {
    PADNE_TRY(periodic_require("padne_periodic_predict", ctx, pd));
    PADNE_REQUIRE(pd->have_r0, "padne_periodic_predict follows padne_periodic_residual");
    PADNE_REQUIRE(n_coef >= 0 && n_coef <= pd->n_vec, "more coefficients than basis vectors");
    PADNE_REQUIRE((n_coef == 0 || coef) && max_out && vertex_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    Scratch sc(ctx);
    double *d_coef = nullptr;
    PADNE_TRY(periodic_upload(pd, sc, n_coef, coef, -1.0, &d_coef));
    return periodic_top(pd, sc, pd->r0, n_coef, d_coef, max_out, vertex_out);
}

extern "C" int padne_periodic_combine(padne_ctx *ctx, padne_periodic *pd, int32_t n_y, const double *y) {
    PADNE_TRY(periodic_require("padne_periodic_combine", ctx, pd));
    PADNE_REQUIRE(pd->marked, "padne_periodic_combine follows padne_periodic_mark");
    PADNE_REQUIRE(n_y >= 0 && n_y <= pd->n_vec, "more coefficients than basis vectors");
    PADNE_REQUIRE(n_y == 0 || y, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    Scratch sc(ctx);
    double *d_y = nullptr;
    PADNE_TRY(periodic_upload(pd, sc, n_y, y, 1.0, &d_y));
    if (pd->n_pot > 0) {
        hipLaunchKernelGGL(periodic_combine_kernel, dim3(nblk(pd->n_pot), (unsigned)pd->n_cols), dim3(256), 0, ctx->stream, pd->n_pot,
                           pd->n_cols, n_y, pd->max_vectors, (const double *)pd->x0, (const double *)d_y, (const double *)pd->V,
                           pd->tr->theta);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return periodic_restart(pd);
}

extern "C" int padne_periodic_vector(padne_ctx *ctx, const padne_periodic *pd, int32_t j, double *out) {
    PADNE_TRY(periodic_require("padne_periodic_vector", ctx, pd));
    PADNE_REQUIRE(j >= -2 && j < pd->n_vec, "no such vector yet (-1: r0, -2: x0)");
    PADNE_REQUIRE(j != -1 || pd->have_r0, "padne_periodic_vector of r0 follows padne_periodic_residual");
    PADNE_REQUIRE(j != -2 || pd->marked, "padne_periodic_vector of x0 follows padne_periodic_mark");
    if (periodic_count(pd) == 0) return PADNE_OK;
    PADNE_REQUIRE(out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const double *src = j == -1 ? pd->r0 : j == -2 ? pd->x0 : periodic_vector(pd, j);
    PADNE_HIP_CHECK(hipMemcpyAsync(out, src, sizeof(double) * periodic_count(pd), hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_periodic_put(padne_ctx *ctx, padne_periodic *pd, int32_t j, const double *in) {
    PADNE_TRY(periodic_require("padne_periodic_put", ctx, pd));
    PADNE_REQUIRE(j >= -3 && j <= pd->n_vec && j < pd->max_vectors, "the next basis vector at the most (-1: r0, -2: x0, -3: the state)");
    PADNE_REQUIRE(in != nullptr || periodic_count(pd) == 0, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    double *dst = j == -1 ? pd->r0 : j == -2 ? pd->x0 : j == -3 ? pd->tr->theta : periodic_vector(pd, j);
    if (periodic_count(pd) > 0)
        PADNE_HIP_CHECK(hipMemcpyAsync(dst, in, sizeof(double) * periodic_count(pd), hipMemcpyHostToDevice, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (j == -1) pd->have_r0 = true;
    if (j == -2) pd->marked = true;
    if (j == -3) return periodic_restart(pd);
    if (j >= 0 && j + 1 > pd->n_vec) pd->n_vec = j + 1;
    return PADNE_OK;
}
