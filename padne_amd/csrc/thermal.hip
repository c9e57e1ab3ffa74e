// Steady-state temperature rise of the copper from Joule heating ("Thermal").  No reference counterpart.
//
// Unknown: theta = T - T_ambient at the first n_potential unknowns of the electrical system (the vertices of the connected
// meshes, then the internal nodes).  One more sheet problem on the meshes the assembled system L keeps on the device:
//
//     A theta = b,    A = K_kappa + diag(h_m(v) M_v) + links
//
//   K_kappa  the cotangent stiffness of the assembly (|cot|/2 weights) with the thermal sheet conductance kappa_m [W/K] of
//            each mesh in the place of sigma, positive sign: padne_assemble_system on L's device arrays, negated;
//   M_v      = sum over the faces incident to v, in ascending global face number, of A_f / 3 (A_f: error_area);
//   h_m      the film coefficient of the mesh [W/(K length^2)]: every loss from the sheet to ambient;
//   links    a thermal conductance g [W/K] per lumped resistor, stamped like the resistor itself;
//   b_v      = sum over the faces incident to v, ascending, of P_f / 3, then the node-heat triples in list order, with
//            P_f = sigma sum_edges w_ik (V_i - V_k)^2 the face's Joule power in the weights' form (face_edge_power).
//
// K and the links annihilate constants, so sum_v h M_v theta_v = sum_v b_v: the film loss equals the heat put in.
//
// Every kernel is a gather or a stream bound by memory: one thread per vertex or face, workgroups of 256, per-column arrays
// field-major ([column][vertex], [column][face]) so the lanes of a wave read and write neighbouring doubles.  No
// floating-point atomics; the sums of the report go through the fixed-order tile reductions of error.hpp: two calls give
// the same bits.  Compiled with -ffp-contract=off: the expressions round as written, a numpy restatement reproduces them.
#include "thermal.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace padne {

// ---- setup ---------------------------------------------------------------------------------------------------------------
// area[t] = A_f
__global__ __launch_bounds__(256) void thermal_area_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                           const double *__restrict__ xy, const long long *__restrict__ voff,
                                                           const long long *__restrict__ toff, double *__restrict__ area,
                                                           int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1, g2, g3;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        area[t] = 0.0;
        return;
    }
    area[t] = error_area(xy[2 * g1], xy[2 * g1 + 1], xy[2 * g2], xy[2 * g2 + 1], xy[2 * g3], xy[2 * g3 + 1]);
}

// Mv[v] = sum of A_f / 3 down the list of v, front to back; hM[v] = h_m Mv[v].  One thread per vertex
__global__ __launch_bounds__(256) void thermal_lump_kernel(const long long n_vert, const int n_mesh, const long long *__restrict__ voff,
                                                           const double *__restrict__ film, const int *__restrict__ vptr,
                                                           const int *__restrict__ vface, const double *__restrict__ area,
                                                           double *__restrict__ Mv, double *__restrict__ hM) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    double s = 0.0;
    for (int e = vptr[v], e1 = vptr[v + 1]; e < e1; ++e) s += area[vface[e]] / 3;
    Mv[v] = s;
    hM[v] = film[find_segment(voff, n_mesh, v)] * s;
}

// K -> A in place: every stored entry negated, and the stored diagonal of vertex i becomes the one rounded sum
// (-K_ii) + hM[i].  One thread per row; a row without a stored diagonal sets *err (an unknown nothing conducts to)
__global__ __launch_bounds__(256) void thermal_form_kernel(const long long n_rows, const long long n_vert,
                                                           const int32_t *__restrict__ rowptr, const int32_t *__restrict__ cols,
                                                           double *__restrict__ vals, const double *__restrict__ hM,
                                                           int *__restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    bool found = false;
    for (int e = rowptr[i], e1 = rowptr[i + 1]; e < e1; ++e) {
        double a = -vals[e];
        if (cols[e] == i) {
            if (i < n_vert) a = a + hM[i];
            found = true;
        }
        vals[e] = a;
    }
    if (!found) *(volatile int *)err = 1;
}

// ---- heat load -----------------------------------------------------------------------------------------------------------
// P[c][t] = sigma sum_edges w_ik (V_i - V_k)^2 of every column c of V[..][n_cols], the arithmetic of
// current_cases_face_kernel's per-mesh power.  One thread per face: corners, xy and weights once, the columns in register
// chunks whose gathers are in flight together.  SCALED (the electro-thermal coupling): the one product sigma[m] * scale[t] in
// the place of sigma[m].  ld: the columns of the block V (n_cols of them are taken, from the column V points at)
template <bool SCALED>
__global__ __launch_bounds__(256) void thermal_face_power_kernel(const long long n_tri, const int n_mesh,
                                                                 const int32_t *__restrict__ tri, const double *__restrict__ xy,
                                                                 const long long *__restrict__ voff,
                                                                 const long long *__restrict__ toff,
                                                                 const double *__restrict__ sigma,
                                                                 const double *__restrict__ scale, const int n_cols,
                                                                 const int ld, const double *__restrict__ V,
                                                                 double *__restrict__ P,
                                                                 int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1, g2, g3;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        for (int c = 0; c < n_cols; ++c) P[(long long)c * n_tri + t] = 0.0;
        return;
    }
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    const double s = SCALED ? sigma[m] * scale[t] : sigma[m];
    const double w23 = cot_half(x2, y2, x3, y3, x1, y1);     // edge 2-3, opposite 1
    const double w31 = cot_half(x3, y3, x1, y1, x2, y2);
    const double w12 = cot_half(x1, y1, x2, y2, x3, y3);
    const double *p1 = V + g1 * ld, *p2 = V + g2 * ld, *p3 = V + g3 * ld;
    for (int j0 = 0; j0 < n_cols; j0 += kThermalChunk) {
        double f1[kThermalChunk], f2[kThermalChunk], f3[kThermalChunk];
#pragma unroll
        for (int q = 0; q < kThermalChunk; ++q)
            if (j0 + q < n_cols) {
                f1[q] = p1[j0 + q];
                f2[q] = p2[j0 + q];
                f3[q] = p3[j0 + q];
            }
#pragma unroll
        for (int q = 0; q < kThermalChunk; ++q)
            if (j0 + q < n_cols) P[(long long)(j0 + q) * n_tri + t] = face_edge_power(s, w12, w23, w31, f1[q], f2[q], f3[q]);
    }
}

// b[q][i] = sum of P[q][f] / 3 down the list of vertex i, front to back, for the nq <= kThermalChunk columns that start at P
// and b; 0 for an unknown that is no vertex.  One thread per unknown, one walk of its list for all columns
__global__ __launch_bounds__(256) void thermal_load_kernel(const long long n_pot, const long long n_vert, const long long n_tri,
                                                           const int *__restrict__ vptr, const int *__restrict__ vface,
                                                           const int nq, const double *__restrict__ P, double *__restrict__ b) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    double acc[kThermalChunk];
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q) acc[q] = 0.0;
    if (i < n_vert)
        for (int e = vptr[i], e1 = vptr[i + 1]; e < e1; ++e) {
            const long long t = vface[e];
#pragma unroll
            for (int q = 0; q < kThermalChunk; ++q)
                if (q < nq) acc[q] += P[(long long)q * n_tri + t] / 3;
        }
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q)
        if (q < nq) b[(long long)q * n_pot + i] = acc[q];
}

// the node-heat triples, grouped by destination (column, unknown) with their list order kept inside a group: one thread per
// destination adds its own, in that order.  Sums into different destinations do not meet, so every b has the bits of the
// triples added one after the other down the list
__global__ __launch_bounds__(256) void thermal_heat_kernel(const int n_groups, const int *__restrict__ group_ptr,
                                                           const long long *__restrict__ group_dst, const double *__restrict__ val,
                                                           double *__restrict__ b) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const long long at = group_dst[g];
    double a = b[at];
    for (int e = group_ptr[g], e1 = group_ptr[g + 1]; e < e1; ++e) a = a + val[e];
    b[at] = a;
}

// ---- report --------------------------------------------------------------------------------------------------------------
// Per face of a tile (256 faces of one mesh, the layout of error_indicator_kernel) and column c: mean[c][t] = ((theta_1 +
// theta_2) + theta_3) / 3 in the corner order of error_corners (mean null: not written), and per tile tile_P[c][b] = the sum
// of P[c][t] in the fixed order of error.hpp
__global__ __launch_bounds__(256) void thermal_report_face_kernel(const int n_mesh, const long long *__restrict__ tile_off,
                                                                  const int32_t *__restrict__ tri, const long long *__restrict__ voff,
                                                                  const long long *__restrict__ toff, const long long n_tri,
                                                                  const long long n_pot, const long long n_blocks, const int n_cols,
                                                                  const double *__restrict__ theta, const double *__restrict__ P,
                                                                  double *__restrict__ mean, double *__restrict__ tile_P) {
    __shared__ double red[4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    long long g1 = 0, g2 = 0, g3 = 0;
    const bool live = t < toff[m + 1];
    const bool ok = live && error_corners(tri, voff, m, t, g1, g2, g3);     // (an index out of range was refused at creation)
    for (int c = 0; c < n_cols; ++c) {
        double p = 0.0;
        if (live) {
            p = P[(long long)c * n_tri + t];
            if (mean != nullptr) {
                const double *th = theta + (long long)c * n_pot;
                mean[(long long)c * n_tri + t] = ok ? ((th[g1] + th[g2]) + th[g3]) / 3 : 0.0;
            }
        }
        p = error_wave_sum(p);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = p;
        __syncthreads();
        if (threadIdx.x == 0) tile_P[(long long)c * n_blocks + b] = error_sum4(red);
        __syncthreads();
    }
}

// Per vertex of a tile (256 vertices of one mesh) and column c: per tile the film loss sum of hM[v] theta[c][v] in the fixed
// order of error.hpp and the largest theta with its vertex (the lowest on a tie).  Per vertex, unless env is null: env[v] =
// max_c theta[c][v] and env_case[v] the lowest c that attains it, sequentially from column 0, replaced on strictly greater
__global__ __launch_bounds__(256) void thermal_report_vertex_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                                    const long long *__restrict__ voff, const long long n_pot,
                                                                    const long long n_blocks, const int n_cols,
                                                                    const double *__restrict__ theta, const double *__restrict__ hM,
                                                                    double *__restrict__ tile_loss, double *__restrict__ tile_max,
                                                                    long long *__restrict__ tile_vert, double *__restrict__ env,
                                                                    int *__restrict__ env_case) {
    __shared__ double red_s[4], red_v[4];
    __shared__ long long red_f[4];
    const long long b = blockIdx.x;
    const int m = find_segment(vtile_off, n_mesh, b);
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    const bool live = v < voff[m + 1];
    const double hm = live ? hM[v] : 0.0;
    double e = 0.0;
    int ec = 0;
    for (int c = 0; c < n_cols; ++c) {
        double loss = 0.0, a = -INFINITY;
        long long f = kErrNoFace;
        if (live) {
            const double th = theta[(long long)c * n_pot + v];
            loss = hm * th;
            a = th;
            f = v;
            if (c == 0 || th > e) {
                e = th;
                ec = c;
            }
        }
        loss = error_wave_sum(loss);
        error_wave_top(a, f);
        if ((threadIdx.x & 63) == 0) {
            red_s[threadIdx.x >> 6] = loss;
            red_v[threadIdx.x >> 6] = a;
            red_f[threadIdx.x >> 6] = f;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
            tile_loss[(long long)c * n_blocks + b] = error_sum4(red_s);
            tile_max[(long long)c * n_blocks + b] = a;
            tile_vert[(long long)c * n_blocks + b] = f;
        }
        __syncthreads();
    }
    if (live && env != nullptr) {
        env[v] = e;
        env_case[v] = ec;
    }
}

// Per (mesh m = blockIdx.x, column c = blockIdx.y), over the mesh's tiles in a fixed order (strided partial sums, then the
// wave and workgroup order of error.hpp): out_sum[c][m] = the sum of tile_sum[c][..]; unless tile_v is null, out_v[c][m] =
// the largest tile_v and out_f[c][m] its index (the lowest on a tie; -infinity and -1 for a mesh without tiles)
__global__ __launch_bounds__(256) void thermal_fold_kernel(const int n_mesh, const long long n_blocks, const long long *__restrict__ tile_off,
                                                           const double *__restrict__ tile_sum, const double *__restrict__ tile_v,
                                                           const long long *__restrict__ tile_f, double *__restrict__ out_sum,
                                                           double *__restrict__ out_v, long long *__restrict__ out_f) {
    __shared__ double red_s[4], red_v[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    const long long at = (long long)blockIdx.y * n_blocks;
    const bool top = tile_v != nullptr;
    double s = 0.0, a = -INFINITY;
    long long f = kErrNoFace;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) {
        s += tile_sum[at + i];
        if (top) error_merge(a, f, tile_v[at + i], tile_f[at + i]);
    }
    s = error_wave_sum(s);
    error_wave_top(a, f);
    if ((threadIdx.x & 63) == 0) {
        red_s[threadIdx.x >> 6] = s;
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long to = (long long)blockIdx.y * n_mesh + m;
        out_sum[to] = error_sum4(red_s);
        if (top) {
            for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
            out_v[to] = a;
            out_f[to] = f == kErrNoFace ? -1 : f;
        }
    }
}

// tiles of 256 items per segment of `off`: tile[m] .. tile[m + 1] are segment m's
std::vector<long long> thermal_tiles(const std::vector<int64_t> &off) {
    std::vector<long long> tile(off.size(), 0);
    for (size_t m = 0; m + 1 < off.size(); ++m) tile[m + 1] = tile[m] + (off[m + 1] - off[m] + 255) / 256;
    return tile;
}

static int thermal_bad_flag(hipStream_t s, const int *d_bad, const char *what) {
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: %s", what);
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}

static void thermal_free(padne_thermal *th) {
    if (th == nullptr) return;
    padne_ctx *ctx = th->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    if (th->A != nullptr) padne_csr_destroy(th->A);
    if (th->stack != nullptr) stack_free(ctx, th->stack);
    if (th->sources != nullptr) sources_free(ctx, th->sources);
    if (th->film != nullptr) film_free(ctx, th->film);
    for (void *p : {(void *)th->vptr, (void *)th->vface, (void *)th->Mv, (void *)th->hM, (void *)th->P, (void *)th->theta})
        if (p != nullptr) pool_free(ctx, p);
    delete th;
}

// a device array of the handle that grows on demand (the old one goes back to the pool; the stream orders its reuse)
static int thermal_reserve(padne_ctx *ctx, double **p, size_t *cap, size_t count) {
    if (count == 0) count = 1;
    if (*p != nullptr && *cap >= count) return PADNE_OK;
    if (*p != nullptr) pool_free(ctx, *p);
    *cap = 0;
    *p = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (*p == nullptr) return PADNE_E_NOMEM;
    *cap = count;
    return PADNE_OK;
}

int thermal_require(const char *entry, padne_ctx *ctx, const padne_thermal *th) {
    PADNE_REQUIRE(ctx && th, "null argument");
    PADNE_REQUIRE(th->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    return PADNE_OK;
}

// b[n_cols][n_pot] on the device from the face powers th->P[n_cols][n_tri] and the node-heat triples: the gather through the
// vertex lists, 8 columns per launch, then the triples, then the heat sources of a handle that has some.  Returns once the
// host lists have been read
int thermal_form_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node,
                             const int32_t *heat_col, const double *heat_val, double *d_b) {
    hipStream_t s = ctx->stream;
    const long long n_pot = th->n_pot;
    // the triples by destination, their order within a destination kept (a stable sort on the host: O(#triples log))
    std::vector<int64_t> order((size_t)n_heat);
    std::iota(order.begin(), order.end(), (int64_t)0);
    auto key = [&](int64_t e) { return (long long)heat_col[e] * n_pot + heat_node[e]; };
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
    std::vector<int> group_ptr;
    std::vector<long long> group_dst;
    std::vector<double> val((size_t)n_heat);
    for (int64_t i = 0; i < n_heat; ++i) {
        const long long k = key(order[(size_t)i]);
        if (i == 0 || k != group_dst.back()) {
            group_ptr.push_back((int)i);
            group_dst.push_back(k);
        }
        val[(size_t)i] = heat_val[order[(size_t)i]];
    }
    group_ptr.push_back((int)n_heat);
    const int n_groups = (int)group_dst.size();
    for (int c0 = 0; c0 < n_cols; c0 += kThermalChunk) {
        const int nq = n_cols - c0 < kThermalChunk ? n_cols - c0 : kThermalChunk;
        hipLaunchKernelGGL(thermal_load_kernel, dim3(nblk(n_pot)), dim3(256), 0, s, n_pot, th->n_vert, th->n_tri, (const int *)th->vptr,
                           (const int *)th->vface, nq, (const double *)(th->P + (size_t)c0 * (size_t)th->n_tri),
                           d_b + (size_t)c0 * (size_t)n_pot);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_heat > 0) {
        Scratch sc(ctx);
        double *d_val = nullptr;
        int *d_ptr = nullptr;
        long long *d_dst = nullptr;
        PADNE_TRY(sc.alloc(&d_ptr, (size_t)n_groups + 1));
        PADNE_TRY(sc.alloc(&d_dst, (size_t)n_groups));
        PADNE_TRY(sc.alloc(&d_val, (size_t)n_heat));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_ptr, group_ptr.data(), sizeof(int) * ((size_t)n_groups + 1), hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_dst, group_dst.data(), sizeof(long long) * (size_t)n_groups, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_val, val.data(), sizeof(double) * (size_t)n_heat, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(thermal_heat_kernel, dim3(nblk(n_groups)), dim3(256), 0, s, n_groups, (const int *)d_ptr,
                           (const long long *)d_dst, (const double *)d_val, d_b);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipStreamSynchronize(s));       // (the copies read the host vectors above before they go)
    }
    return sources_add_load(ctx, th, n_cols, d_b);      // the handle's heat sources, if it has any (sources.hip)
}

// What follows the face powers th->P[n_cols][n_tri]: b, the block solve, theta home.  PADNE_E_NOTCONVERGED still keeps and
// returns the iterate.  On a handle with film curves (film.hip; one column): the load is kept, the linearisation's c is added
// to it, and the iteration starts from the iterate the film was linearised about; `resolve`: the kept load in the place of a
// new one
int thermal_solve_core(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node,
                       const int32_t *heat_col, const double *heat_val, const padne_solve_opts *opts, double *theta_host,
                       padne_solve_info *info, bool resolve) {
    hipStream_t s = ctx->stream;
    const long long n_pot = th->n_pot;
    PADNE_TRY(thermal_reserve(ctx, &th->theta, &th->theta_cap, (size_t)n_cols * (size_t)n_pot));
    Scratch sc(ctx);
    double *d_b = nullptr;
    PADNE_TRY(sc.alloc(&d_b, (size_t)n_cols * (size_t)n_pot));
    th->solved = false;
    padne_film *fm = th->film;
    const size_t pot_bytes = sizeof(double) * (size_t)n_pot;
    if (resolve) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_b, fm->b0, pot_bytes, hipMemcpyDeviceToDevice, s));
    } else {
        PADNE_TRY(thermal_form_load(ctx, th, n_cols, n_heat, heat_node, heat_col, heat_val, d_b));
        if (fm != nullptr) {
            PADNE_HIP_CHECK(hipMemcpyAsync(fm->b0, d_b, pot_bytes, hipMemcpyDeviceToDevice, s));
            fm->have_load = true;
        }
    }
    const bool warm = fm != nullptr && fm->warm;
    if (fm != nullptr) PADNE_TRY(film_add_load(ctx, th, d_b));
    if (warm) PADNE_HIP_CHECK(hipMemcpyAsync(th->theta, fm->lin, pot_bytes, hipMemcpyDeviceToDevice, s));
    else PADNE_HIP_CHECK(hipMemsetAsync(th->theta, 0, sizeof(double) * (size_t)n_cols * (size_t)n_pot, s));
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
    o.flags &= ~1;                                      // theta starts from zero: a zero column comes back as exact zeros
    if (warm) o.flags |= 1;                             // (film curves: from the iterate of the last linearise)
    const int rc = padne_solve_spd_dev(ctx, th->A, d_b, th->theta, n_cols, &o, info);
    if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
    th->n_cols = n_cols;
    th->solved = true;
    if (theta_host != nullptr)
        PADNE_HIP_CHECK(hipMemcpyAsync(theta_host, th->theta, sizeof(double) * (size_t)n_cols * (size_t)n_pot, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
}

int thermal_check_heat(const padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node,
                              const int32_t *heat_col, const double *heat_val) {
    PADNE_REQUIRE(n_cols >= 1 && n_cols <= 4096, "between 1 and 4096 columns");
    PADNE_REQUIRE(n_heat >= 0 && n_heat <= 0x7fffffffLL, "number of node-heat triples");
    PADNE_REQUIRE(n_heat == 0 || (heat_node && heat_col && heat_val), "null argument");
    for (int64_t e = 0; e < n_heat; ++e) {
        PADNE_REQUIRE(heat_node[e] >= 0 && heat_node[e] < th->n_pot, "node-heat unknown out of range");
        PADNE_REQUIRE(heat_col[e] >= 0 && heat_col[e] < n_cols, "node-heat column out of range");
        PADNE_REQUIRE(std::isfinite(heat_val[e]), "node heat must be finite");
    }
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_thermal_create(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int32_t n_mesh, const double *kappa,
                                    const double *film, int64_t n_link, const int64_t *link_a, const int64_t *link_b,
                                    const double *link_g, padne_thermal **out) {
    PADNE_REQUIRE(ctx && L && out && kappa && film, "null argument");
    PADNE_REQUIRE(L->mesh_n_mesh > 0 && L->mesh_xy != nullptr,
                  "the system matrix does not carry a mesh (only padne_assemble_system keeps it)");
    PADNE_REQUIRE(n_mesh == L->mesh_n_mesh, "n_mesh must be that of the system's mesh");
    PADNE_REQUIRE(n_potential >= L->mesh_n_vert && n_potential <= L->n_rows, "n_potential: the vertices, then the internal nodes");
    PADNE_REQUIRE(n_link >= 0 && n_link <= 0x1fffffffLL, "number of links");
    PADNE_REQUIRE(n_link == 0 || (link_a && link_b && link_g), "null argument");
    for (int m = 0; m < n_mesh; ++m) {
        PADNE_REQUIRE(std::isfinite(kappa[m]) && kappa[m] > 0.0, "the thermal sheet conductance of every mesh must be finite and positive");
        PADNE_REQUIRE(std::isfinite(film[m]) && film[m] > 0.0, "the film coefficient of every mesh must be finite and positive");
    }
    // a link is stamped like the resistor it stands for (solver.py:475-478), in the reference's sign: K is negated afterwards
    std::vector<int64_t> row, col;
    std::vector<double> val;
    for (int64_t e = 0; e < n_link; ++e) {
        const int64_t a = link_a[e], b = link_b[e];
        const double g = link_g[e];
        PADNE_REQUIRE(a >= 0 && a < n_potential && b >= 0 && b < n_potential, "link terminal out of range");
        PADNE_REQUIRE(std::isfinite(g) && g >= 0.0, "a link conductance must be finite and not negative");
        if (g == 0.0) continue;                         // no thermal path
        row.insert(row.end(), {a, a, b, b});
        col.insert(col.end(), {a, b, b, a});
        val.insert(val.end(), {-g, g, -g, g});
    }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_thermal *th = new padne_thermal;
    th->ctx = ctx;
    th->L = L;
    th->n_pot = n_potential;
    th->n_vert = L->mesh_n_vert;
    th->n_tri = L->mesh_n_tri;
    th->n_mesh = n_mesh;
    th->film_host.assign(film, film + n_mesh);
    struct Guard {
        padne_thermal *th;
        ~Guard() { thermal_free(th); }
    } guard{th};
    th->voff.assign((size_t)n_mesh + 1, 0);
    th->toff.assign((size_t)n_mesh + 1, 0);
    PADNE_HIP_CHECK(hipMemcpyAsync(th->voff.data(), L->mesh_voff, sizeof(int64_t) * ((size_t)n_mesh + 1), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(th->toff.data(), L->mesh_toff, sizeof(int64_t) * ((size_t)n_mesh + 1), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    // K: the assembly over L's device-resident mesh with kappa for sigma; only the offset tables and the stamps are host data
    PADNE_TRY(padne_assemble_system_ex(ctx, n_potential, th->n_vert, L->mesh_xy, th->n_tri, L->mesh_tri, n_mesh, th->voff.data(),
                                       th->toff.data(), kappa, (int64_t)row.size(), row.data(), col.data(), val.data(), 0, &th->A));
    const ErrorMesh M = error_mesh_of(L);
    PADNE_TRY(error_vertex_faces(ctx, M, &th->vptr, &th->vface));
    th->Mv = (double *)pool_alloc(ctx, sizeof(double) * (size_t)(th->n_vert > 0 ? th->n_vert : 1));
    th->hM = (double *)pool_alloc(ctx, sizeof(double) * (size_t)(th->n_vert > 0 ? th->n_vert : 1));
    if (th->Mv == nullptr || th->hM == nullptr) return PADNE_E_NOMEM;
    Scratch sc(ctx);
    double *d_area = nullptr, *d_film = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_area, (size_t)th->n_tri));
    PADNE_TRY(sc.alloc(&d_film, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_bad, 2));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, 2 * sizeof(int), s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_film, film, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    if (th->n_tri > 0) {
        hipLaunchKernelGGL(thermal_area_kernel, dim3(nblk(th->n_tri)), dim3(256), 0, s, th->n_tri, n_mesh, M.tri, M.xy, M.voff, M.toff,
                           d_area, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (th->n_vert > 0) {
        hipLaunchKernelGGL(thermal_lump_kernel, dim3(nblk(th->n_vert)), dim3(256), 0, s, th->n_vert, n_mesh, M.voff,
                           (const double *)d_film, (const int *)th->vptr, (const int *)th->vface, (const double *)d_area, th->Mv, th->hM);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_potential > 0) {
        hipLaunchKernelGGL(thermal_form_kernel, dim3(nblk(n_potential)), dim3(256), 0, s, (long long)n_potential, th->n_vert,
                           (const int32_t *)th->A->rowptr, (const int32_t *)th->A->cols, th->A->vals, (const double *)th->hM, d_bad + 1);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_TRY(thermal_bad_flag(s, d_bad, "triangle index out of range"));
    PADNE_TRY(thermal_bad_flag(s, d_bad + 1, "an unknown of the thermal system has no diagonal: a vertex without a face of non-zero "
                                             "area, or an internal node that no link of positive conductance reaches"));
    guard.th = nullptr;
    *out = th;
    return PADNE_OK;
}

extern "C" int padne_thermal_destroy(padne_thermal *th) {
    thermal_free(th);
    return PADNE_OK;
}

extern "C" int padne_thermal_matrix(const padne_thermal *th, const padne_csr **csr_out) {
    PADNE_REQUIRE(th && csr_out, "null argument");
    *csr_out = th->A;
    return PADNE_OK;
}

extern "C" int padne_thermal_lumped(padne_ctx *ctx, const padne_thermal *th, double *M_out) {
    PADNE_TRY(thermal_require("padne_thermal_lumped", ctx, th));
    if (th->n_vert == 0) return PADNE_OK;
    PADNE_REQUIRE(M_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(M_out, th->Mv, sizeof(double) * (size_t)th->n_vert, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

// the face powers of the caller on the device, in the handle's array (any earlier solve's results are no longer reported)
int padne::thermal_upload_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host) {
    PADNE_REQUIRE(th->n_tri == 0 || face_power_host != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t count = (size_t)n_cols * (size_t)th->n_tri;
    th->solved = false;
    PADNE_TRY(thermal_reserve(ctx, &th->P, &th->P_cap, count));
    if (count > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(th->P, face_power_host, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
        PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PADNE_OK;
}

extern "C" int padne_thermal_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host, int64_t n_heat,
                                  const int64_t *heat_node, const int32_t *heat_col, const double *heat_val, double *b_out) {
    PADNE_TRY(thermal_require("padne_thermal_load", ctx, th));
    PADNE_TRY(thermal_check_heat(th, n_cols, n_heat, heat_node, heat_col, heat_val));
    PADNE_REQUIRE(b_out != nullptr, "null argument");
    PADNE_TRY(thermal_upload_power(ctx, th, n_cols, face_power_host));
    Scratch sc(ctx);
    double *d_b = nullptr;
    PADNE_TRY(sc.alloc(&d_b, (size_t)n_cols * (size_t)th->n_pot));
    PADNE_TRY(thermal_form_load(ctx, th, n_cols, n_heat, heat_node, heat_col, heat_val, d_b));
    PADNE_HIP_CHECK(hipMemcpyAsync(b_out, d_b, sizeof(double) * (size_t)n_cols * (size_t)th->n_pot, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_thermal_solve(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host, int64_t n_heat,
                                   const int64_t *heat_node, const int32_t *heat_col, const double *heat_val,
                                   const padne_solve_opts *opts, double *theta_host, padne_solve_info *info) {
    PADNE_TRY(thermal_require("padne_thermal_solve", ctx, th));
    PADNE_TRY(film_refuses("padne_thermal_solve", th, n_cols));
    PADNE_TRY(thermal_check_heat(th, n_cols, n_heat, heat_node, heat_col, heat_val));
    PADNE_TRY(thermal_upload_power(ctx, th, n_cols, face_power_host));
    return thermal_solve_core(ctx, th, n_cols, n_heat, heat_node, heat_col, heat_val, opts, theta_host, info);
}

static int thermal_face_power_of(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int32_t ld, const double *V, const double *scale);

// the checks of an entry that reads the block `plan`'s last padne_kkt_finish_block left on the device: *V_out that block
int padne::thermal_kkt_block(const char *entry, padne_ctx *ctx, const padne_thermal *th, padne_kkt *plan, int32_t n_cols,
                             const double **V_out) {
    PADNE_TRY(thermal_require(entry, ctx, th));
    long long N = 0;
    const padne_csr *L = nullptr;
    PADNE_TRY(kkt_finished_block(entry, ctx, plan, n_cols, V_out, &N, &L));
    PADNE_REQUIRE(L == th->L, "the plan and the thermal model must come from the same assembled system");
    return PADNE_OK;
}

// th->P[n_cols][n_tri] from the block V of thermal_kkt_block (scale as in thermal_solve_kkt_scaled)
int padne::thermal_kkt_face_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *V, const double *scale) {
    return thermal_face_power_of(ctx, th, n_cols, n_cols, V, scale);
}

int padne::thermal_kkt_face_power_column(padne_ctx *ctx, padne_thermal *th, int32_t ld, int32_t col, const double *V,
                                         const double *scale) {
    return thermal_face_power_of(ctx, th, 1, ld, V + col, scale);
}

static int thermal_face_power_of(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int32_t ld, const double *V, const double *scale) {
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    th->solved = false;
    PADNE_TRY(thermal_reserve(ctx, &th->P, &th->P_cap, (size_t)n_cols * (size_t)th->n_tri));
    if (th->n_tri > 0) {
        const ErrorMesh M = error_mesh_of(th->L);
        Scratch sc(ctx);
        int *d_bad = nullptr;
        PADNE_TRY(sc.alloc(&d_bad, 1));
        PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
        if (scale != nullptr)
            hipLaunchKernelGGL(thermal_face_power_kernel<true>, dim3(nblk(th->n_tri)), dim3(256), 0, s, th->n_tri, th->n_mesh, M.tri,
                               M.xy, M.voff, M.toff, M.sigma, scale, (int)n_cols, (int)ld, V, th->P, d_bad);
        else
            hipLaunchKernelGGL(thermal_face_power_kernel<false>, dim3(nblk(th->n_tri)), dim3(256), 0, s, th->n_tri, th->n_mesh, M.tri,
                               M.xy, M.voff, M.toff, M.sigma, (const double *)nullptr, (int)n_cols, (int)ld, V, th->P, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_TRY(thermal_bad_flag(s, d_bad, "triangle index out of range"));
    }
    return PADNE_OK;
}

int padne::thermal_solve_kkt_scaled(const char *entry, padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols,
                                    const double *scale, int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col,
                                    const double *heat_val, const padne_solve_opts *opts, double *theta_host,
                                    padne_solve_info *info) {
    const double *V = nullptr;
    PADNE_TRY(thermal_kkt_block(entry, ctx, th, plan, n_cols, &V));
    PADNE_TRY(film_refuses(entry, th, n_cols));
    PADNE_TRY(thermal_check_heat(th, n_cols, n_heat, heat_node, heat_col, heat_val));
    PADNE_TRY(thermal_kkt_face_power(ctx, th, n_cols, V, scale));
    return thermal_solve_core(ctx, th, n_cols, n_heat, heat_node, heat_col, heat_val, opts, theta_host, info);
}

extern "C" int padne_thermal_solve_kkt(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols, int64_t n_heat,
                                       const int64_t *heat_node, const int32_t *heat_col, const double *heat_val,
                                       const padne_solve_opts *opts, double *theta_host, padne_solve_info *info) {
    return thermal_solve_kkt_scaled("padne_thermal_solve_kkt", ctx, th, plan, n_cols, nullptr, n_heat, heat_node, heat_col, heat_val,
                                    opts, theta_host, info);
}

extern "C" int padne_thermal_face_power(padne_ctx *ctx, const padne_thermal *th, int32_t n_cols, double *out_host) {
    PADNE_TRY(thermal_require("padne_thermal_face_power", ctx, th));
    PADNE_REQUIRE(th->solved && n_cols == th->n_cols, "padne_thermal_face_power follows a solve of as many columns");
    if (th->n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(out_host != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(out_host, th->P, sizeof(double) * (size_t)n_cols * (size_t)th->n_tri, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

extern "C" int padne_thermal_report(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_tri, int64_t n_vert, int32_t n_mesh,
                                    double *face_mean_out, double *mesh_max_out, int64_t *mesh_vertex_out, double *mesh_heat_out,
                                    double *mesh_loss_out, double *env_out, int32_t *env_case_out) {
    PADNE_TRY(thermal_require("padne_thermal_report", ctx, th));
    PADNE_REQUIRE(th->solved && n_cols == th->n_cols, "padne_thermal_report follows a solve of as many columns");
    PADNE_REQUIRE(n_tri == th->n_tri && n_vert == th->n_vert && n_mesh == th->n_mesh,
                  "n_tri, n_vert and n_mesh must be those of the system's mesh");
    PADNE_REQUIRE(mesh_max_out && mesh_vertex_out && mesh_heat_out && mesh_loss_out, "null argument");
    PADNE_REQUIRE((env_out == nullptr) == (env_case_out == nullptr), "env_out and env_case_out are given or left out together");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const std::vector<long long> ftile = thermal_tiles(th->toff), vtile = thermal_tiles(th->voff);
    const long long n_fb = ftile[(size_t)n_mesh], n_vb = vtile[(size_t)n_mesh];
    PADNE_REQUIRE(n_fb <= 0x7fffffffLL && n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const size_t nc = (size_t)n_cols, nm = (size_t)n_mesh, nfb = (size_t)(n_fb > 0 ? n_fb : 1), nvb = (size_t)(n_vb > 0 ? n_vb : 1);
    const bool means = face_mean_out != nullptr && n_tri > 0, envelope = env_out != nullptr && n_vert > 0;
    const ErrorMesh M = error_mesh_of(th->L);
    Scratch sc(ctx);
    long long *d_ftile = nullptr, *d_vtile = nullptr, *d_tvert = nullptr, *d_mvert = nullptr;
    double *d_mean = nullptr, *d_tP = nullptr, *d_tloss = nullptr, *d_tmax = nullptr, *d_env = nullptr, *d_heat = nullptr,
           *d_loss = nullptr, *d_max = nullptr;
    int *d_case = nullptr;
    PADNE_TRY(sc.alloc(&d_ftile, nm + 1));
    PADNE_TRY(sc.alloc(&d_vtile, nm + 1));
    if (means) PADNE_TRY(sc.alloc(&d_mean, nc * (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_tP, nc * nfb));
    PADNE_TRY(sc.alloc(&d_tloss, nc * nvb));
    PADNE_TRY(sc.alloc(&d_tmax, nc * nvb));
    PADNE_TRY(sc.alloc(&d_tvert, nc * nvb));
    if (envelope) {
        PADNE_TRY(sc.alloc(&d_env, (size_t)n_vert));
        PADNE_TRY(sc.alloc(&d_case, (size_t)n_vert));
    }
    PADNE_TRY(sc.alloc(&d_heat, nc * nm));
    PADNE_TRY(sc.alloc(&d_loss, nc * nm));
    PADNE_TRY(sc.alloc(&d_max, nc * nm));
    PADNE_TRY(sc.alloc(&d_mvert, nc * nm));
    // (pageable host memory: the copies are staged before the call returns, so the tables may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ftile, ftile.data(), sizeof(long long) * (nm + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_vtile, vtile.data(), sizeof(long long) * (nm + 1), hipMemcpyHostToDevice, s));
    if (n_fb > 0) {
        hipLaunchKernelGGL(thermal_report_face_kernel, dim3((unsigned)n_fb), dim3(256), 0, s, (int)n_mesh, (const long long *)d_ftile, M.tri,
                           M.voff, M.toff, (long long)n_tri, th->n_pot, n_fb, (int)n_cols, (const double *)th->theta,
                           (const double *)th->P, d_mean, d_tP);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_vb > 0) {
        hipLaunchKernelGGL(thermal_report_vertex_kernel, dim3((unsigned)n_vb), dim3(256), 0, s, (int)n_mesh, (const long long *)d_vtile,
                           M.voff, th->n_pot, n_vb, (int)n_cols, (const double *)th->theta, (const double *)th->hM, d_tloss, d_tmax,
                           d_tvert, d_env, d_case);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(thermal_fold_kernel, dim3((unsigned)n_mesh, (unsigned)n_cols), dim3(256), 0, s, (int)n_mesh, n_fb,
                       (const long long *)d_ftile, (const double *)d_tP, (const double *)nullptr, (const long long *)nullptr, d_heat,
                       (double *)nullptr, (long long *)nullptr);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(thermal_fold_kernel, dim3((unsigned)n_mesh, (unsigned)n_cols), dim3(256), 0, s, (int)n_mesh, n_vb,
                       (const long long *)d_vtile, (const double *)d_tloss, (const double *)d_tmax, (const long long *)d_tvert, d_loss,
                       d_max, d_mvert);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_heat_out, d_heat, sizeof(double) * nc * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_loss_out, d_loss, sizeof(double) * nc * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_max, sizeof(double) * nc * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_vertex_out, d_mvert, sizeof(long long) * nc * nm, hipMemcpyDeviceToHost, s));
    if (means) PADNE_HIP_CHECK(hipMemcpyAsync(face_mean_out, d_mean, sizeof(double) * nc * (size_t)n_tri, hipMemcpyDeviceToHost, s));
    if (envelope) {
        PADNE_HIP_CHECK(hipMemcpyAsync(env_out, d_env, sizeof(double) * (size_t)n_vert, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(env_case_out, d_case, sizeof(int32_t) * (size_t)n_vert, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}
