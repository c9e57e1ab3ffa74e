// Goal-oriented (dual-weighted) error estimator over the faces ("Goal-oriented error").  No reference
// counterpart.  Field 0 is the solution x (column 0 of V[..][n_cols]), field 1 + j the adjoint lambda_j = sum_m W[j][m] V[:, m]
// of objective j, combined per corner in registers as sensitivity_block_kernel combines it.  Every field a goes through
// the passes of error.hip -- g_f^a, G_v^a, the midpoint differences m_ab^a, eta_f^a -- and field 0 is paired with each
// adjoint:
//   delta_jf = sigma (A_f / 3) (m_12^0 . m_12^(1+j) + m_23^0 . m_23^(1+j) + m_31^0 . m_31^(1+j))     (signed)
//   omega_jf = eta_f^0 eta_f^(1+j)                                                                   (>= |delta_jf|)
// and per (mesh, objective) the sums of both and the face with the largest omega (the lower face on a tie).
// The arithmetic is error.hpp's, shared with error.hip: field 0's G, eta, E_m, P_m, largest eta and face are the bits of
// padne_kkt_error_estimate.  Objectives go in chunks of kGoalChunk per launch; field 0 is recomputed with every chunk (it
// is 1 field in 9) and its results are stored by the first chunk only.  Per-field arrays are field-major ([plane][face],
// [plane][vertex], plane = 2 field + component), so the lanes of a wave read and write neighbouring doubles.  Three passes
// bound by memory and one fold, no floating-point atomics, every sum in a fixed order: two calls give the same bits.
#include "error.hpp"

#include <cmath>
#include <vector>

namespace padne {

constexpr int kGoalChunk = 8;       // objectives per launch
constexpr int kGoalCols = 8;        // columns of V read per step of the combination (kPowerChunk of fields.hip)

// g[2 f][t], g[2 f + 1][t] = the face gradient of field f = 0 .. nq, area[t] = A_f.  One thread per face: each corner's row of
// V is read once.  W null: field 1 + q is column 1 + j0 + q itself.  power (unless null): sigma |g^0|^2 with the arithmetic of
// power_density_kernel
__global__ __launch_bounds__(256) void goal_face_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                        const double *__restrict__ xy, const long long *__restrict__ voff,
                                                        const long long *__restrict__ toff, const double *__restrict__ sigma,
                                                        const int n_cols, const double *__restrict__ V,
                                                        const double *__restrict__ W, double *__restrict__ power, const int j0,
                                                        const int nq, double *__restrict__ g, double *__restrict__ area,
                                                        int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1, g2, g3;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        for (int p = 0; p < 2 * (1 + nq); ++p) g[(long long)p * n_tri + t] = 0.0;
        area[t] = 0.0;
        if (power != nullptr) power[t] = 0.0;
        return;
    }
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    const double *p1 = V + g1 * n_cols, *p2 = V + g2 * n_cols, *p3 = V + g3 * n_cols;
    double a1[kGoalChunk], a2[kGoalChunk], a3[kGoalChunk];
#pragma unroll
    for (int q = 0; q < kGoalChunk; ++q) a1[q] = a2[q] = a3[q] = 0.0;
    double u1 = p1[0], u2 = p2[0], u3 = p3[0];
    if (W != nullptr) {
        for (int c0 = 0; c0 < n_cols; c0 += kGoalCols) {
            double f1[kGoalCols], f2[kGoalCols], f3[kGoalCols];
#pragma unroll
            for (int c = 0; c < kGoalCols; ++c)
                if (c0 + c < n_cols) {
                    f1[c] = p1[c0 + c];
                    f2[c] = p2[c0 + c];
                    f3[c] = p3[c0 + c];
                }
#pragma unroll
            for (int q = 0; q < kGoalChunk; ++q)
                if (q < nq) {
                    const double *w = W + (long long)(j0 + q) * n_cols + c0;
#pragma unroll
                    for (int c = 0; c < kGoalCols; ++c)
                        if (c0 + c < n_cols) {
                            a1[q] += w[c] * f1[c];
                            a2[q] += w[c] * f2[c];
                            a3[q] += w[c] * f3[c];
                        }
                }
        }
    } else {
#pragma unroll
        for (int q = 0; q < kGoalChunk; ++q)
            if (q < nq) {
                a1[q] = p1[1 + j0 + q];
                a2[q] = p2[1 + j0 + q];
                a3[q] = p3[1 + j0 + q];
            }
    }
    double gx, gy;
    face_gradient_of(x1, y1, x2, y2, x3, y3, u1, u2, u3, gx, gy);
    g[t] = gx;
    g[n_tri + t] = gy;
    if (power != nullptr) power[t] = face_power_of(gx, gy, sigma[m]);
    area[t] = error_area(x1, y1, x2, y2, x3, y3);
#pragma unroll
    for (int q = 0; q < kGoalChunk; ++q)
        if (q < nq) {
            face_gradient_of(x1, y1, x2, y2, x3, y3, a1[q], a2[q], a3[q], gx, gy);
            g[(long long)(2 * (1 + q)) * n_tri + t] = gx;
            g[(long long)(2 * (1 + q) + 1) * n_tri + t] = gy;
        }
}

// G of every field at every vertex from one walk of the vertex's list, front to back: field 0 into G0[v][2] (the layout of
// error_recover_kernel), field 1 + q into Gd[2 q][v], Gd[2 q + 1][v]
__global__ __launch_bounds__(256) void goal_recover_kernel(const long long n_vert, const long long n_tri, const int *__restrict__ vptr,
                                                           const int *__restrict__ vface, const int nq,
                                                           const double *__restrict__ g, const double *__restrict__ area,
                                                           double *__restrict__ G0, double *__restrict__ Gd) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    double sx[1 + kGoalChunk], sy[1 + kGoalChunk], sa = 0.0;
#pragma unroll
    for (int f = 0; f < 1 + kGoalChunk; ++f) sx[f] = sy[f] = 0.0;
    for (int e = vptr[v], e1 = vptr[v + 1]; e < e1; ++e) {
        const long long t = vface[e];
        const double a = area[t];
#pragma unroll
        for (int f = 0; f < 1 + kGoalChunk; ++f)
            if (f <= nq) error_recover_add(sx[f], sy[f], g[(long long)(2 * f) * n_tri + t], g[(long long)(2 * f + 1) * n_tri + t], a);
        sa += a;
    }
    error_recover_end(sx[0], sy[0], sa, G0[2 * v], G0[2 * v + 1]);
#pragma unroll
    for (int q = 0; q < kGoalChunk; ++q)
        if (q < nq) error_recover_end(sx[1 + q], sy[1 + q], sa, Gd[(long long)(2 * q) * n_vert + v], Gd[(long long)(2 * q + 1) * n_vert + v]);
}

// Per face of a tile (256 faces of one mesh, the layout of error_indicator_kernel): eta of field 0 and of the nq adjoints,
// delta and omega of the nq pairs; per tile, in a fixed order, field 0's partials as error_indicator_kernel writes them
// and per pair the sums of omega and delta and the largest omega with its face.  eta0 null: field 0's results are not
// stored (a later chunk).  The per-pair arrays start at this chunk's first objective: [q][n_tri] and [q][n_blocks]
__global__ __launch_bounds__(256) void goal_indicator_kernel(
    const int n_mesh, const long long *__restrict__ tile_off, const int32_t *__restrict__ tri, const long long *__restrict__ voff,
    const long long *__restrict__ toff, const double *__restrict__ sigma, const long long n_tri, const long long n_vert,
    const long long n_blocks, const int nq, const double *__restrict__ g, const double *__restrict__ area,
    const double *__restrict__ G0, const double *__restrict__ Gd, double *__restrict__ eta0, double *__restrict__ tile_E,
    double *__restrict__ tile_P, double *__restrict__ tile_max, long long *__restrict__ tile_face, double *__restrict__ eta,
    double *__restrict__ delta, double *__restrict__ omega, double *__restrict__ tile_om, double *__restrict__ tile_de,
    double *__restrict__ tile_top, long long *__restrict__ tile_tf) {
    __shared__ double red_E[4], red_P[4], red_v[4];
    __shared__ long long red_f[4];
    __shared__ double red_om[kGoalChunk][4], red_de[kGoalChunk][4], red_tv[kGoalChunk][4];
    __shared__ long long red_tf[kGoalChunk][4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    long long g1 = 0, g2 = 0, g3 = 0;
    const bool live = t < toff[m + 1];
    const bool ok = live && error_corners(tri, voff, m, t, g1, g2, g3);   // (an index out of range was reported by goal_face_kernel)
    double e2 = 0.0, p = 0.0, a = -1.0, value = 0.0, s = 0.0, ar = 0.0;
    long long f = kErrNoFace;
    double m0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
        const double gx = g[t], gy = g[n_tri + t];
        ar = area[t];
        s = sigma[m];
        error_midpoints(G0[2 * g1], G0[2 * g1 + 1], G0[2 * g2], G0[2 * g2 + 1], G0[2 * g3], G0[2 * g3 + 1], gx, gy, m0);
        e2 = error_midpoint_form(s, ar, m0, m0);
        p = error_power(s, ar, gx, gy);
        value = sqrt(e2);
    }
    if (live) {
        if (eta0 != nullptr) eta0[t] = value;
        a = value;
        f = t;
    }
    const int w = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    e2 = error_wave_sum(e2);
    p = error_wave_sum(p);
    error_wave_top(a, f);
    if (lead) {
        red_E[w] = e2;
        red_P[w] = p;
        red_v[w] = a;
        red_f[w] = f;
    }
#pragma unroll
    for (int q = 0; q < kGoalChunk; ++q) {
        if (q >= nq) break;
        double om = 0.0, de = 0.0, tv = -1.0;
        long long tf = kErrNoFace;
        if (live) {
            double ev = 0.0;
            if (ok) {
                const double *Gx = Gd + (long long)(2 * q) * n_vert, *Gy = Gd + (long long)(2 * q + 1) * n_vert;
                double mq[6];
                error_midpoints(Gx[g1], Gy[g1], Gx[g2], Gy[g2], Gx[g3], Gy[g3], g[(long long)(2 * (1 + q)) * n_tri + t],
                                g[(long long)(2 * (1 + q) + 1) * n_tri + t], mq);
                ev = sqrt(error_midpoint_form(s, ar, mq, mq));
                de = error_midpoint_form(s, ar, m0, mq);
                om = value * ev;
            }
            eta[(long long)q * n_tri + t] = ev;
            delta[(long long)q * n_tri + t] = de;
            omega[(long long)q * n_tri + t] = om;
            tv = om;
            tf = t;
        }
        om = error_wave_sum(om);
        de = error_wave_sum(de);
        error_wave_top(tv, tf);
        if (lead) {
            red_om[q][w] = om;
            red_de[q][w] = de;
            red_tv[q][w] = tv;
            red_tf[q][w] = tf;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && eta0 != nullptr) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        tile_E[b] = error_sum4(red_E);
        tile_P[b] = error_sum4(red_P);
        tile_max[b] = a;
        tile_face[b] = f;
    }
    if ((int)threadIdx.x < nq) {
        const int q = threadIdx.x;
        double tv = red_tv[q][0];
        long long tf = red_tf[q][0];
        for (int r = 1; r < 4; ++r) error_merge(tv, tf, red_tv[q][r], red_tf[q][r]);
        tile_om[(long long)q * n_blocks + b] = error_sum4(red_om[q]);
        tile_de[(long long)q * n_blocks + b] = error_sum4(red_de[q]);
        tile_top[(long long)q * n_blocks + b] = tv;
        tile_tf[(long long)q * n_blocks + b] = tf;
    }
}

// error_mesh_fold for item y = blockIdx.y of n_items: two sums and a top over the tiles of mesh blockIdx.x, tile arrays
// [item][n_blocks] and results [item][n_mesh].  One workgroup per (mesh, item)
__global__ __launch_bounds__(256) void goal_fold_kernel(const int n_mesh, const long long n_blocks, const long long *__restrict__ tile_off,
                                                        const double *__restrict__ tile_a, const double *__restrict__ tile_b,
                                                        const double *__restrict__ tile_v, const long long *__restrict__ tile_f,
                                                        double *__restrict__ out_a, double *__restrict__ out_b,
                                                        double *__restrict__ out_v, long long *__restrict__ out_f) {
    __shared__ double red_a[4], red_b[4], red_v[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    const long long y = blockIdx.y, at = y * n_blocks, to = y * n_mesh + m;
    error_fold_tiles(tile_off, m, tile_a + at, tile_b + at, tile_v + at, tile_f + at, red_a, red_b, red_v, red_f, out_a + to, out_b + to,
                     out_v + to, out_f + to);
}

// The passes over the mesh M with its lists, for the fields of V_dev[..][n_cols] and W_dev[n_obj][n_cols] (null: field 1 + j
// is column 1 + j); toff_host[n_mesh + 1] are M's triangle offsets on the host.  Asynchronous, like launch_error_estimate
int launch_goal_error(padne_ctx *ctx, const ErrorMesh &M, const long long *toff_host, const int *vptr, const int *vface, int n_cols,
                      int n_obj, const double *W_dev, const double *V_dev, const GoalOut &out, int *bad_dev) {
    hipStream_t s = ctx->stream;
    PADNE_REQUIRE(n_obj >= 1 && n_cols >= 1 && (W_dev != nullptr || n_cols >= 1 + n_obj), "fields and columns");
    std::vector<long long> tile((size_t)M.n_mesh + 1, 0);
    for (int m = 0; m < M.n_mesh; ++m) {
        PADNE_REQUIRE(toff_host[m + 1] >= toff_host[m], "mesh triangle offsets");
        tile[(size_t)m + 1] = tile[(size_t)m] + (toff_host[m + 1] - toff_host[m] + 255) / 256;
    }
    const long long n_blocks = tile[(size_t)M.n_mesh];
    PADNE_REQUIRE(n_blocks <= 0x7fffffffLL, "too many triangles for one launch");
    const size_t nb = (size_t)(n_blocks > 0 ? n_blocks : 1), nt = (size_t)(M.n_tri > 0 ? M.n_tri : 1),
                 nv = (size_t)(M.n_vert > 0 ? M.n_vert : 1);
    const int chunk = n_obj < kGoalChunk ? n_obj : kGoalChunk;
    Scratch sc(ctx);
    long long *d_tile = nullptr, *d_tface = nullptr, *d_ttf = nullptr;
    double *d_g = nullptr, *d_area = nullptr, *d_Gd = nullptr, *d_tE = nullptr, *d_tP = nullptr, *d_tmax = nullptr, *d_tom = nullptr,
           *d_tde = nullptr, *d_ttop = nullptr;
    PADNE_TRY(sc.alloc(&d_tile, (size_t)M.n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_g, 2 * (size_t)(1 + chunk) * nt));
    PADNE_TRY(sc.alloc(&d_area, nt));
    PADNE_TRY(sc.alloc(&d_Gd, 2 * (size_t)chunk * nv));
    PADNE_TRY(sc.alloc(&d_tE, nb));
    PADNE_TRY(sc.alloc(&d_tP, nb));
    PADNE_TRY(sc.alloc(&d_tmax, nb));
    PADNE_TRY(sc.alloc(&d_tface, nb));
    PADNE_TRY(sc.alloc(&d_tom, (size_t)chunk * nb));
    PADNE_TRY(sc.alloc(&d_tde, (size_t)chunk * nb));
    PADNE_TRY(sc.alloc(&d_ttop, (size_t)chunk * nb));
    PADNE_TRY(sc.alloc(&d_ttf, (size_t)chunk * nb));
    // (pageable host memory: the copy is staged before the call returns, so `tile` may go)
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tile, tile.data(), sizeof(long long) * ((size_t)M.n_mesh + 1), hipMemcpyHostToDevice, s));
    for (int j0 = 0; j0 < n_obj; j0 += kGoalChunk) {
        const int nq = n_obj - j0 < kGoalChunk ? n_obj - j0 : kGoalChunk;
        const bool first = j0 == 0;
        if (M.n_tri > 0) {
            hipLaunchKernelGGL(goal_face_kernel, dim3(nblk(M.n_tri)), dim3(256), 0, s, M.n_tri, M.n_mesh, M.tri, M.xy, M.voff, M.toff,
                               M.sigma, n_cols, V_dev, W_dev, first ? out.power : (double *)nullptr, j0, nq, d_g, d_area, bad_dev);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        if (M.n_vert > 0) {
            hipLaunchKernelGGL(goal_recover_kernel, dim3(nblk(M.n_vert)), dim3(256), 0, s, M.n_vert, M.n_tri, vptr, vface, nq,
                               (const double *)d_g, (const double *)d_area, out.G0, d_Gd);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        if (n_blocks > 0) {
            hipLaunchKernelGGL(goal_indicator_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, M.n_mesh, (const long long *)d_tile, M.tri,
                               M.voff, M.toff, M.sigma, M.n_tri, M.n_vert, n_blocks, nq, (const double *)d_g, (const double *)d_area,
                               (const double *)out.G0, (const double *)d_Gd, first ? out.eta0 : (double *)nullptr, d_tE, d_tP, d_tmax,
                               d_tface, out.eta + (size_t)j0 * (size_t)M.n_tri, out.delta + (size_t)j0 * (size_t)M.n_tri,
                               out.omega + (size_t)j0 * (size_t)M.n_tri, d_tom, d_tde, d_ttop, d_ttf);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        if (first) {
            hipLaunchKernelGGL(goal_fold_kernel, dim3((unsigned)M.n_mesh, 1), dim3(256), 0, s, M.n_mesh, n_blocks, (const long long *)d_tile,
                               (const double *)d_tE, (const double *)d_tP, (const double *)d_tmax, (const long long *)d_tface, out.mesh_E,
                               out.mesh_P, out.mesh_max, out.mesh_face);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(goal_fold_kernel, dim3((unsigned)M.n_mesh, (unsigned)nq), dim3(256), 0, s, M.n_mesh, n_blocks,
                           (const long long *)d_tile, (const double *)d_tom, (const double *)d_tde, (const double *)d_ttop,
                           (const long long *)d_ttf, out.obj_omega + (size_t)j0 * (size_t)M.n_mesh,
                           out.obj_delta + (size_t)j0 * (size_t)M.n_mesh, out.obj_top + (size_t)j0 * (size_t)M.n_mesh,
                           out.obj_face + (size_t)j0 * (size_t)M.n_mesh);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return PADNE_OK;
}

int csr_goal_error(padne_ctx *ctx, const padne_csr *L, int **vptr, int **vface, int n_cols, int n_obj, const double *W_dev,
                   const double *V_dev, const GoalOut &out, int *bad_dev) {
    const ErrorMesh M = error_mesh_of(L);
    if (*vptr == nullptr) PADNE_TRY(error_vertex_faces(ctx, M, vptr, vface));
    std::vector<long long> toff((size_t)M.n_mesh + 1);
    PADNE_HIP_CHECK(hipMemcpyAsync(toff.data(), M.toff, sizeof(long long) * ((size_t)M.n_mesh + 1), hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return launch_goal_error(ctx, M, toff.data(), *vptr, *vface, n_cols, n_obj, W_dev, V_dev, out, bad_dev);
}

}  // namespace padne

using namespace padne;

// The standalone form: meshes and n_fields columns of potentials from the host, field 0 paired with each of the others; the
// lists are built for this call
extern "C" int padne_goal_error(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                                int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                                const double *conductance, int32_t n_fields, const double *potential_host, double *power_out,
                                double *G_out, double *eta_out, double *mesh_error_out, double *mesh_power_out, double *mesh_max_out,
                                int64_t *mesh_face_out, double *dual_eta_out, double *delta_out, double *omega_out,
                                double *mesh_omega_out, double *mesh_delta_out, double *mesh_top_out, int64_t *mesh_top_face_out) {
    PADNE_REQUIRE(ctx, "ctx");
    PADNE_REQUIRE(n_vert >= 0 && n_tri >= 0 && n_mesh > 0 && n_mesh <= 0x7fffffffLL, "sizes: at least one mesh, nothing negative");
    PADNE_REQUIRE(n_fields >= 2 && n_fields <= 4097, "between 2 and 4097 fields");
    PADNE_REQUIRE(mesh_vertex_offset && mesh_tri_offset && conductance, "null argument");
    PADNE_REQUIRE(mesh_error_out && mesh_power_out && mesh_max_out && mesh_face_out, "null argument");
    PADNE_REQUIRE(mesh_omega_out && mesh_delta_out && mesh_top_out && mesh_top_face_out, "null argument");
    PADNE_REQUIRE(n_vert == 0 || (xy_host && potential_host && G_out), "null argument");
    PADNE_REQUIRE(n_tri == 0 || (tri_host && power_out && eta_out && dual_eta_out && delta_out && omega_out), "null argument");
    PADNE_REQUIRE(mesh_vertex_offset[0] == 0 && mesh_tri_offset[0] == 0, "offset tables must start at 0");
    PADNE_REQUIRE(mesh_vertex_offset[n_mesh] == n_vert && mesh_tri_offset[n_mesh] == n_tri, "offset tables");
    for (int64_t m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(mesh_vertex_offset[m] <= mesh_vertex_offset[m + 1] && mesh_tri_offset[m] <= mesh_tri_offset[m + 1],
                      "offset tables not monotone");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n_obj = (size_t)n_fields - 1, nt = (size_t)n_tri, nv = (size_t)n_vert, nm = (size_t)n_mesh;
    Scratch sc(ctx);
    double *d_xy = nullptr, *d_sigma = nullptr, *d_pot = nullptr;
    int32_t *d_tri = nullptr;
    int *d_bad = nullptr, *vptr = nullptr, *vface = nullptr;
    long long *d_voff = nullptr, *d_toff = nullptr;
    GoalOut out;
    PADNE_TRY(sc.alloc(&d_xy, 2 * nv));
    PADNE_TRY(sc.alloc(&d_pot, nv * (size_t)n_fields));
    PADNE_TRY(sc.alloc(&d_tri, 3 * nt));
    PADNE_TRY(sc.alloc(&d_sigma, nm));
    PADNE_TRY(sc.alloc(&d_voff, nm + 1));
    PADNE_TRY(sc.alloc(&d_toff, nm + 1));
    PADNE_TRY(sc.alloc(&out.power, nt));
    PADNE_TRY(sc.alloc(&out.G0, 2 * nv));
    PADNE_TRY(sc.alloc(&out.eta0, nt));
    PADNE_TRY(sc.alloc(&out.mesh_E, nm));
    PADNE_TRY(sc.alloc(&out.mesh_P, nm));
    PADNE_TRY(sc.alloc(&out.mesh_max, nm));
    PADNE_TRY(sc.alloc(&out.mesh_face, nm));
    PADNE_TRY(sc.alloc(&out.eta, n_obj * nt));
    PADNE_TRY(sc.alloc(&out.delta, n_obj * nt));
    PADNE_TRY(sc.alloc(&out.omega, n_obj * nt));
    PADNE_TRY(sc.alloc(&out.obj_omega, n_obj * nm));
    PADNE_TRY(sc.alloc(&out.obj_delta, n_obj * nm));
    PADNE_TRY(sc.alloc(&out.obj_top, n_obj * nm));
    PADNE_TRY(sc.alloc(&out.obj_face, n_obj * nm));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (n_vert > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_xy, xy_host, sizeof(double) * 2 * nv, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_pot, potential_host, sizeof(double) * nv * (size_t)n_fields, hipMemcpyHostToDevice, s));
    }
    if (n_tri > 0) PADNE_HIP_CHECK(hipMemcpyAsync(d_tri, tri_host, sizeof(int32_t) * 3 * nt, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_sigma, conductance, sizeof(double) * nm, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_voff, mesh_vertex_offset, sizeof(long long) * (nm + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_toff, mesh_tri_offset, sizeof(long long) * (nm + 1), hipMemcpyHostToDevice, s));
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
    PADNE_TRY(launch_goal_error(ctx, M, toff.data(), vptr, vface, n_fields, (int)n_obj, nullptr, d_pot, out, d_bad));
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_error_out, out.mesh_E, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_power_out, out.mesh_P, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, out.mesh_max, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_face_out, out.mesh_face, sizeof(long long) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_omega_out, out.obj_omega, sizeof(double) * n_obj * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_delta_out, out.obj_delta, sizeof(double) * n_obj * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_top_out, out.obj_top, sizeof(double) * n_obj * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_top_face_out, out.obj_face, sizeof(long long) * n_obj * nm, hipMemcpyDeviceToHost, s));
    if (n_vert > 0) PADNE_HIP_CHECK(hipMemcpyAsync(G_out, out.G0, sizeof(double) * 2 * nv, hipMemcpyDeviceToHost, s));
    if (n_tri > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(power_out, out.power, sizeof(double) * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(eta_out, out.eta0, sizeof(double) * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(dual_eta_out, out.eta, sizeof(double) * n_obj * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(delta_out, out.delta, sizeof(double) * n_obj * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(omega_out, out.omega, sizeof(double) * n_obj * nt, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}
