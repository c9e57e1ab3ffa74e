// Gradient-recovery (Zienkiewicz-Zhu) error estimator over the faces ("Error estimate").  No reference
// counterpart.  Per connected mesh m with sheet conductance sigma, faces visited with the corners of power_density_kernel:
//   g_f, A_f   the face gradient of face.hpp and the face's area;
//   G_v        = (sum_f A_f g_f) / (sum_f A_f) over the faces incident to vertex v, in ascending global face number
//                (0 for a vertex without faces or whose areas sum to zero);
//   eta_f^2    = sigma (A_f / 3) (|m_12|^2 + |m_23|^2 + |m_31|^2) with d_c = G_(corner c) - g_f, m_ab = (d_a + d_b) / 2:
//                sigma times the exact integral over f of |G_h - g_f|^2 for the piecewise-linear G_h;
//   E_m, P_m   = sum eta_f^2 and sum sigma A_f |g_f|^2 over the mesh, and its face with the largest eta_f.
// Three passes over the mesh, all bound by memory: error_face_kernel stores (g_f, A_f) once per face, error_recover_kernel
// sums them per vertex through the vertex -> faces lists (one thread per vertex: a store pass and a per-destination sum
// instead of float atomics, so two calls give the same bits), error_indicator_kernel reads three G per face.  The lists
// are a CSR whose rows ascend in face number BY CONSTRUCTION: the (vertex, face) pairs are written in face order and sorted
// by vertex with a stable radix sort; the row pointer is a binary search per vertex.  Nothing is left to the order in
// which atomics land.
#include "error.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <vector>

namespace padne {

// ---- vertex -> incident faces ----------------------------------------------------------------------------------------
// key[3 t + c] = the global vertex of corner c of face t (n_vert for an index out of range: sorted behind every list),
// val[3 t + c] = t: the pairs in ascending face order
__global__ __launch_bounds__(256) void error_pair_kernel(const long long n_tri, const long long n_vert, const int n_mesh,
                                                         const int32_t *__restrict__ tri, const long long *__restrict__ voff,
                                                         const long long *__restrict__ toff, unsigned *__restrict__ key,
                                                         int *__restrict__ val, int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1 = n_vert, g2 = n_vert, g3 = n_vert;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        g1 = g2 = g3 = n_vert;
    }
    key[3 * t] = (unsigned)g1;
    key[3 * t + 1] = (unsigned)g2;
    key[3 * t + 2] = (unsigned)g3;
    val[3 * t] = val[3 * t + 1] = val[3 * t + 2] = (int)t;
}

// ptr[v] = the first position of the sorted keys that holds v or more, v = 0 .. n_vert
__global__ __launch_bounds__(256) void error_ptr_kernel(const long long n_vert, const long long n_pairs,
                                                        const unsigned *__restrict__ key, int *__restrict__ ptr) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v > n_vert) return;
    long long lo = 0, hi = n_pairs;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)key[mid] < v) lo = mid + 1; else hi = mid;
    }
    ptr[v] = (int)lo;
}

// The lists of the mesh: *vptr_out[n_vert + 1], *vface_out[3 n_tri] (pool allocations the caller owns).  Synchronises once,
// for the index check: PADNE_E_INVALID for a triangle index out of range.
int error_vertex_faces(padne_ctx *ctx, const ErrorMesh &M, int **vptr_out, int **vface_out) {
    PADNE_REQUIRE(M.n_vert < 0x7fffffffLL && 3 * M.n_tri <= 0x7fffffffLL, "too many vertices or faces for 32-bit vertex lists");
    hipStream_t s = ctx->stream;
    const long long n_pairs = 3 * M.n_tri;
    Scratch sc(ctx), keep(ctx);
    unsigned *key_a = nullptr, *key_b = nullptr;
    int *val_a = nullptr, *vface = nullptr, *vptr = nullptr, *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&key_a, (size_t)n_pairs));
    PADNE_TRY(sc.alloc(&key_b, (size_t)n_pairs));
    PADNE_TRY(sc.alloc(&val_a, (size_t)n_pairs));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_TRY(keep.alloc(&vface, (size_t)n_pairs));
    PADNE_TRY(keep.alloc(&vptr, (size_t)M.n_vert + 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (M.n_tri > 0) {
        hipLaunchKernelGGL(error_pair_kernel, dim3(nblk(M.n_tri)), dim3(256), 0, s, M.n_tri, M.n_vert, M.n_mesh, M.tri, M.voff, M.toff,
                           key_a, val_a, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
        int key_bits = 1;
        while ((1ll << key_bits) <= M.n_vert) ++key_bits;        // keys run to n_vert inclusive
        // stable: equal vertices keep the order of the pairs, which is the order of the faces
        size_t tmp_bytes = 0;
        PADNE_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_a, key_b, val_a, vface, (size_t)n_pairs, 0, key_bits, s));
        void *tmp = nullptr;
        PADNE_TRY(sc.alloc((char **)&tmp, tmp_bytes));
        PADNE_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, vface, (size_t)n_pairs, 0, key_bits, s));
    }
    hipLaunchKernelGGL(error_ptr_kernel, dim3(nblk(M.n_vert + 1)), dim3(256), 0, s, M.n_vert, n_pairs, (const unsigned *)key_b, vptr);
    PADNE_HIP_CHECK(hipGetLastError());
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    keep.disown(vface);
    keep.disown(vptr);
    *vptr_out = vptr;
    *vface_out = vface;
    return PADNE_OK;
}

// ---- the three passes ------------------------------------------------------------------------------------------------
// gA[t] = (g_x, g_y, A_f) of every face, from column 0 of V[..][n_cols]
__global__ __launch_bounds__(256) void error_face_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                         const double *__restrict__ xy, const long long *__restrict__ voff,
                                                         const long long *__restrict__ toff, const int n_cols,
                                                         const double *__restrict__ V, double *__restrict__ gA,
                                                         int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1, g2, g3;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        gA[3 * t] = gA[3 * t + 1] = gA[3 * t + 2] = 0.0;
        return;
    }
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    double gx, gy;
    face_gradient_of(x1, y1, x2, y2, x3, y3, V[g1 * n_cols], V[g2 * n_cols], V[g3 * n_cols], gx, gy);
    gA[3 * t] = gx;
    gA[3 * t + 1] = gy;
    gA[3 * t + 2] = error_area(x1, y1, x2, y2, x3, y3);
}

// G[v] = (sum A_f g_f) / (sum A_f) over the list of v, front to back: one thread per vertex
__global__ __launch_bounds__(256) void error_recover_kernel(const long long n_vert, const int *__restrict__ vptr,
                                                            const int *__restrict__ vface, const double *__restrict__ gA,
                                                            double *__restrict__ G) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    double sx = 0.0, sy = 0.0, sa = 0.0;
    for (int e = vptr[v], e1 = vptr[v + 1]; e < e1; ++e) {
        const double *p = gA + 3 * (long long)vface[e];
        const double a = p[2];
        error_recover_add(sx, sy, p[0], p[1], a);
        sa += a;
    }
    error_recover_end(sx, sy, sa, G[2 * v], G[2 * v + 1]);
}

// eta[t], and per tile (256 faces of one mesh, the layout of sensitivity_block_kernel) the sums of eta^2 and of
// sigma A |g|^2 in a fixed order, and the largest eta with its face (-1 and kErrNoFace for a tile without a face)
__global__ __launch_bounds__(256) void error_indicator_kernel(
    const int n_mesh, const long long *__restrict__ tile_off, const int32_t *__restrict__ tri, const long long *__restrict__ voff,
    const long long *__restrict__ toff, const double *__restrict__ sigma, const double *__restrict__ gA, const double *__restrict__ G,
    double *__restrict__ eta, double *__restrict__ tile_E, double *__restrict__ tile_P, double *__restrict__ tile_max,
    long long *__restrict__ tile_face) {
    __shared__ double red_E[4], red_P[4], red_v[4];
    __shared__ long long red_f[4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    long long g1 = 0, g2 = 0, g3 = 0;
    const bool live = t < toff[m + 1];
    double e2 = 0.0, p = 0.0, a = -1.0;
    long long f = kErrNoFace;
    if (live) {
        double value = 0.0;
        if (error_corners(tri, voff, m, t, g1, g2, g3)) {       // (an index out of range was reported by error_face_kernel)
            const double gx = gA[3 * t], gy = gA[3 * t + 1], area = gA[3 * t + 2], s = sigma[m];
            double mid[6];
            error_midpoints(G[2 * g1], G[2 * g1 + 1], G[2 * g2], G[2 * g2 + 1], G[2 * g3], G[2 * g3 + 1], gx, gy, mid);
            e2 = error_midpoint_form(s, area, mid, mid);
            p = error_power(s, area, gx, gy);
            value = sqrt(e2);
        }
        eta[t] = value;
        a = value;
        f = t;
    }
    e2 = error_wave_sum(e2);
    p = error_wave_sum(p);
    error_wave_top(a, f);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_E[w] = e2;
        red_P[w] = p;
        red_v[w] = a;
        red_f[w] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        tile_E[b] = error_sum4(red_E);
        tile_P[b] = error_sum4(red_P);
        tile_max[b] = a;
        tile_face[b] = f;
    }
}

// per mesh, over its tiles in a fixed order: E_m, P_m, the largest eta and its face (global index; -1.0 and -1 for a mesh
// without faces).  One workgroup per mesh
__global__ __launch_bounds__(256) void error_mesh_fold(const long long *__restrict__ tile_off, const double *__restrict__ tile_E,
                                                       const double *__restrict__ tile_P, const double *__restrict__ tile_max,
                                                       const long long *__restrict__ tile_face, double *__restrict__ mesh_E,
                                                       double *__restrict__ mesh_P, double *__restrict__ mesh_max,
                                                       long long *__restrict__ mesh_face) {
    __shared__ double red_E[4], red_P[4], red_v[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    error_fold_tiles(tile_off, m, tile_E, tile_P, tile_max, tile_face, red_E, red_P, red_v, red_f, mesh_E + m, mesh_P + m, mesh_max + m,
                     mesh_face + m);
}

// The three passes and the fold over the mesh M with its lists, from column 0 of V_dev[..][n_cols]; toff_host[n_mesh + 1]
// are M's triangle offsets on the host.  Device outputs: G_dev[n_vert][2], eta_dev[n_tri], mesh_*_dev[n_mesh]; *bad_dev is
// set for a triangle index out of range.  Asynchronous: the scratch goes back to the pool on return, and the context's one
// stream orders its reuse after these launches.
int launch_error_estimate(padne_ctx *ctx, const ErrorMesh &M, const long long *toff_host, const int *vptr, const int *vface,
                          int n_cols, const double *V_dev, double *G_dev, double *eta_dev, double *mesh_E_dev, double *mesh_P_dev,
                          double *mesh_max_dev, long long *mesh_face_dev, int *bad_dev) {
    hipStream_t s = ctx->stream;
    std::vector<long long> tile((size_t)M.n_mesh + 1, 0);
    for (int m = 0; m < M.n_mesh; ++m) {
        PADNE_REQUIRE(toff_host[m + 1] >= toff_host[m], "mesh triangle offsets");
        tile[(size_t)m + 1] = tile[(size_t)m] + (toff_host[m + 1] - toff_host[m] + 255) / 256;
    }
    const long long n_blocks = tile[(size_t)M.n_mesh];
    PADNE_REQUIRE(n_blocks <= 0x7fffffffLL, "too many triangles for one launch");
    const size_t nb = (size_t)(n_blocks > 0 ? n_blocks : 1);
    Scratch sc(ctx);
    long long *d_tile = nullptr, *d_tface = nullptr;
    double *d_gA = nullptr, *d_tE = nullptr, *d_tP = nullptr, *d_tmax = nullptr;
    PADNE_TRY(sc.alloc(&d_tile, (size_t)M.n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_gA, 3 * (size_t)(M.n_tri > 0 ? M.n_tri : 1)));
    PADNE_TRY(sc.alloc(&d_tE, nb));
    PADNE_TRY(sc.alloc(&d_tP, nb));
    PADNE_TRY(sc.alloc(&d_tmax, nb));
    PADNE_TRY(sc.alloc(&d_tface, nb));
    // (pageable host memory: the copy is staged before the call returns, so `tile` may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tile, tile.data(), sizeof(long long) * ((size_t)M.n_mesh + 1), hipMemcpyHostToDevice, s));
    if (M.n_tri > 0) {
        hipLaunchKernelGGL(error_face_kernel, dim3(nblk(M.n_tri)), dim3(256), 0, s, M.n_tri, M.n_mesh, M.tri, M.xy, M.voff, M.toff,
                           n_cols, V_dev, d_gA, bad_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (M.n_vert > 0) {
        hipLaunchKernelGGL(error_recover_kernel, dim3(nblk(M.n_vert)), dim3(256), 0, s, M.n_vert, vptr, vface, (const double *)d_gA,
                           G_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_blocks > 0) {
        hipLaunchKernelGGL(error_indicator_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, M.n_mesh, (const long long *)d_tile,
                           M.tri, M.voff, M.toff, M.sigma, (const double *)d_gA, (const double *)G_dev, eta_dev, d_tE, d_tP, d_tmax,
                           d_tface);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(error_mesh_fold, dim3((unsigned)M.n_mesh), dim3(256), 0, s, (const long long *)d_tile, (const double *)d_tE,
                       (const double *)d_tP, (const double *)d_tmax, (const long long *)d_tface, mesh_E_dev, mesh_P_dev,
                       mesh_max_dev, mesh_face_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

ErrorMesh error_mesh_of(const padne_csr *L) {
    ErrorMesh M;
    M.xy = L->mesh_xy;
    M.sigma = L->mesh_sigma;
    M.tri = L->mesh_tri;
    M.voff = L->mesh_voff;
    M.toff = L->mesh_toff;
    M.n_vert = L->mesh_n_vert;
    M.n_tri = L->mesh_n_tri;
    M.n_mesh = (int)L->mesh_n_mesh;
    return M;
}

// The estimate of the mesh a system keeps, with the lists *vptr / *vface of the caller (built here on first use and left
// with the caller): device results as launch_error_estimate leaves them.  Every call waits once for the mesh's triangle
// offsets to come home (the tile layout is made on the host, as in padne_kkt_current_report); the first also for the lists'
// index check.  The launches themselves are asynchronous.
int csr_error_estimate(padne_ctx *ctx, const padne_csr *L, int **vptr, int **vface, int n_cols, const double *V_dev,
                       double *G_dev, double *eta_dev, double *mesh_E_dev, double *mesh_P_dev, double *mesh_max_dev,
                       long long *mesh_face_dev, int *bad_dev) {
    const ErrorMesh M = error_mesh_of(L);
    if (*vptr == nullptr) PADNE_TRY(error_vertex_faces(ctx, M, vptr, vface));
    std::vector<long long> toff((size_t)M.n_mesh + 1);
    PADNE_HIP_CHECK(hipMemcpyAsync(toff.data(), M.toff, sizeof(long long) * ((size_t)M.n_mesh + 1), hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return launch_error_estimate(ctx, M, toff.data(), *vptr, *vface, n_cols, V_dev, G_dev, eta_dev, mesh_E_dev, mesh_P_dev,
                                 mesh_max_dev, mesh_face_dev, bad_dev);
}

}  // namespace padne

using namespace padne;

// The standalone form: meshes and potentials from the host (padne_power_density's arguments), the lists built for this call.
extern "C" int padne_error_estimate(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                                    int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                                    const double *conductance, const double *potential_host, double *G_out, double *eta_out,
                                    double *mesh_error_out, double *mesh_power_out, double *mesh_max_out, int64_t *mesh_face_out) {
    PADNE_REQUIRE(ctx, "ctx");
    PADNE_REQUIRE(n_vert >= 0 && n_tri >= 0 && n_mesh > 0 && n_mesh <= 0x7fffffffLL, "sizes: at least one mesh, nothing negative");
    PADNE_REQUIRE(mesh_vertex_offset && mesh_tri_offset && conductance, "null argument");
    PADNE_REQUIRE(mesh_error_out && mesh_power_out && mesh_max_out && mesh_face_out, "null argument");
    PADNE_REQUIRE(n_vert == 0 || (xy_host && potential_host && G_out), "null argument");
    PADNE_REQUIRE(n_tri == 0 || (tri_host && eta_out), "null argument");
    PADNE_REQUIRE(mesh_vertex_offset[0] == 0 && mesh_tri_offset[0] == 0, "offset tables must start at 0");
    PADNE_REQUIRE(mesh_vertex_offset[n_mesh] == n_vert && mesh_tri_offset[n_mesh] == n_tri, "offset tables");
    for (int64_t m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(mesh_vertex_offset[m] <= mesh_vertex_offset[m + 1] && mesh_tri_offset[m] <= mesh_tri_offset[m + 1],
                      "offset tables not monotone");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    double *d_xy = nullptr, *d_sigma = nullptr, *d_pot = nullptr, *d_G = nullptr, *d_eta = nullptr, *d_E = nullptr, *d_P = nullptr,
           *d_max = nullptr;
    int32_t *d_tri = nullptr;
    int *d_bad = nullptr, *vptr = nullptr, *vface = nullptr;
    long long *d_voff = nullptr, *d_toff = nullptr, *d_face = nullptr;
    PADNE_TRY(sc.alloc(&d_xy, 2 * (size_t)n_vert));
    PADNE_TRY(sc.alloc(&d_pot, (size_t)n_vert));
    PADNE_TRY(sc.alloc(&d_G, 2 * (size_t)n_vert));
    PADNE_TRY(sc.alloc(&d_tri, 3 * (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_eta, (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_sigma, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_voff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_toff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_E, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_P, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_max, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_face, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (n_vert > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_xy, xy_host, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_pot, potential_host, sizeof(double) * (size_t)n_vert, hipMemcpyHostToDevice, s));
    }
    if (n_tri > 0) PADNE_HIP_CHECK(hipMemcpyAsync(d_tri, tri_host, sizeof(int32_t) * 3 * (size_t)n_tri, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_sigma, conductance, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_voff, mesh_vertex_offset, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_toff, mesh_tri_offset, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    ErrorMesh M;
    M.xy = d_xy;
    M.sigma = d_sigma;
    M.tri = d_tri;
    M.voff = d_voff;
    M.toff = d_toff;
    M.n_vert = n_vert;
    M.n_tri = n_tri;
    M.n_mesh = (int)n_mesh;
    PADNE_TRY(error_vertex_faces(ctx, M, &vptr, &vface));
    sc.ptrs.push_back(vptr);                                      // this call's own lists: back to the pool with the rest
    sc.ptrs.push_back(vface);
    std::vector<long long> toff(mesh_tri_offset, mesh_tri_offset + n_mesh + 1);
    PADNE_TRY(launch_error_estimate(ctx, M, toff.data(), vptr, vface, 1, d_pot, d_G, d_eta, d_E, d_P, d_max, d_face, d_bad));
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_error_out, d_E, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_power_out, d_P, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_max, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_face_out, d_face, sizeof(long long) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    if (n_vert > 0) PADNE_HIP_CHECK(hipMemcpyAsync(G_out, d_G, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyDeviceToHost, s));
    if (n_tri > 0) PADNE_HIP_CHECK(hipMemcpyAsync(eta_out, d_eta, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}
