// What the gradient-recovery estimator (error.hip) and the goal-oriented estimator (goal.hip) share: the mesh they run over,
// the corner order, and every piece of arithmetic whose bits the two must agree on -- the face's area, the recovery sum of
// a vertex, the edge-midpoint differences of a face, eta^2, the power, and the fixed-order reductions of a 256-thread
// workgroup.  Both translation units are compiled with -ffp-contract=off, so an expression written once here rounds the
// same way in both.
#pragma once

#include "common.hpp"
#include "face.hpp"

namespace padne {

// the mesh the passes run over: device arrays, as padne_csr keeps them
struct ErrorMesh {
    const double *xy = nullptr, *sigma = nullptr;
    const int32_t *tri = nullptr;
    const long long *voff = nullptr, *toff = nullptr;
    long long n_vert = 0, n_tri = 0;
    int n_mesh = 0;
};

constexpr long long kErrNoFace = 0x7fffffffffffffffLL;

// (eta, face) pairs: the larger eta wins, the lower face on a tie
__device__ __forceinline__ void error_merge(double &v, long long &f, double ov, long long of) {
    if (ov > v || (ov == v && of < f)) {
        v = ov;
        f = of;
    }
}

// the global corners of face t of mesh m in the order power_density_kernel visits them; false for an index out of range
__device__ __forceinline__ bool error_corners(const int32_t *__restrict__ tri, const long long *__restrict__ voff, int m,
                                              long long t, long long &g1, long long &g2, long long &g3) {
    const long long v0 = voff[m];
    const long long nv = voff[m + 1] - v0;
    const int l1 = tri[3 * t + 2], l2 = tri[3 * t], l3 = tri[3 * t + 1];
    if (l1 < 0 || l2 < 0 || l3 < 0 || l1 >= nv || l2 >= nv || l3 >= nv) return false;
    g1 = v0 + l1;
    g2 = v0 + l2;
    g3 = v0 + l3;
    return true;
}

// A_f
__device__ __forceinline__ double error_area(double x1, double y1, double x2, double y2, double x3, double y3) {
    return fabs((x2 - x1) * (y3 - y1) - (y2 - y1) * (x3 - x1)) / 2;
}

// one face (g, a) of a vertex's recovery sum, and the quotient that ends it
__device__ __forceinline__ void error_recover_add(double &sx, double &sy, double gx, double gy, double a) {
    sx += a * gx;
    sy += a * gy;
}

__device__ __forceinline__ void error_recover_end(double sx, double sy, double sa, double &Gx, double &Gy) {
    const bool some = sa > 0.0;
    Gx = some ? sx / sa : 0.0;
    Gy = some ? sy / sa : 0.0;
}

// m[0..5] = (m_12, m_23, m_31) of a face with gradient g and the recovered gradients G1, G2, G3 of its corners
__device__ __forceinline__ void error_midpoints(double G1x, double G1y, double G2x, double G2y, double G3x, double G3y, double gx,
                                                double gy, double *m) {
    const double d1x = G1x - gx, d1y = G1y - gy;
    const double d2x = G2x - gx, d2y = G2y - gy;
    const double d3x = G3x - gx, d3y = G3y - gy;
    m[0] = (d1x + d2x) / 2; m[1] = (d1y + d2y) / 2;
    m[2] = (d2x + d3x) / 2; m[3] = (d2y + d3y) / 2;
    m[4] = (d3x + d1x) / 2; m[5] = (d3y + d1y) / 2;
}

// sigma (A_f / 3) (m_12 . n_12 + m_23 . n_23 + m_31 . n_31): eta_f^2 for n = m, the goal estimator's delta otherwise
__device__ __forceinline__ double error_midpoint_form(double s, double area, const double *m, const double *n) {
    return s * (area / 3) * (((m[0] * n[0] + m[1] * n[1]) + (m[2] * n[2] + m[3] * n[3])) + (m[4] * n[4] + m[5] * n[5]));
}

// sigma A_f |g_f|^2
__device__ __forceinline__ double error_power(double s, double area, double gx, double gy) {
    return s * area * (gx * gx + gy * gy);
}

// The sums and tops of a 256-thread workgroup in a fixed order: down each wave of 64 by halving strides, lane 0 of every
// wave holds the wave's, and the four waves are joined as (0 + 1) + (2 + 3), tops from wave 0 to wave 3.
__device__ __forceinline__ double error_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ void error_wave_top(double &a, long long &f) {
    for (int off = 32; off > 0; off >>= 1) error_merge(a, f, __shfl_down(a, off, 64), __shfl_down(f, off, 64));
}

__device__ __forceinline__ double error_sum4(const double *red) { return (red[0] + red[1]) + (red[2] + red[3]); }

// Two sums and a top over the tiles tile_off[m] .. tile_off[m + 1] of one mesh, by one workgroup: out_a, out_b the sums of
// tile_a and tile_b, out_v the largest tile_v with its tile_f (-1.0 and -1 for a mesh without faces).  red_*: 4 entries
// of shared memory each
__device__ __forceinline__ void error_fold_tiles(const long long *__restrict__ tile_off, const int m, const double *__restrict__ tile_a,
                                                 const double *__restrict__ tile_b, const double *__restrict__ tile_v,
                                                 const long long *__restrict__ tile_f, double *red_a, double *red_b, double *red_v,
                                                 long long *red_f, double *out_a, double *out_b, double *out_v, long long *out_f) {
    double sa = 0.0, sb = 0.0, a = -1.0;
    long long f = kErrNoFace;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) {
        sa += tile_a[i];
        sb += tile_b[i];
        error_merge(a, f, tile_v[i], tile_f[i]);
    }
    sa = error_wave_sum(sa);
    sb = error_wave_sum(sb);
    error_wave_top(a, f);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_a[w] = sa;
        red_b[w] = sb;
        red_v[w] = a;
        red_f[w] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) error_merge(a, f, red_v[q], red_f[q]);
        *out_a = error_sum4(red_a);
        *out_b = error_sum4(red_b);
        *out_v = a;
        *out_f = f == kErrNoFace ? -1 : f;
    }
}

// The vertex -> faces lists of the mesh (error.hip): *vptr_out[n_vert + 1], *vface_out[3 n_tri], pool allocations the
// caller owns; PADNE_E_INVALID for a triangle index out of range
int error_vertex_faces(padne_ctx *ctx, const ErrorMesh &M, int **vptr_out, int **vface_out);
// the mesh a system keeps
ErrorMesh error_mesh_of(const padne_csr *L);

// Where the goal-oriented estimator (goal.hip) leaves its results, all on the device.  Field 0, as launch_error_estimate
// leaves them: G0[n_vert][2], eta0[n_tri], mesh_E / mesh_P / mesh_max / mesh_face[n_mesh]; and power[n_tri], its power
// density with the arithmetic of power_density_kernel.  Per objective j, objective-major:
// eta[n_obj][n_tri] of the adjoint, delta and omega[n_obj][n_tri], and per mesh their sums and the largest omega with its
// face, obj_*[n_obj][n_mesh]
struct GoalOut {
    double *power = nullptr, *G0 = nullptr, *eta0 = nullptr, *mesh_E = nullptr, *mesh_P = nullptr, *mesh_max = nullptr;
    long long *mesh_face = nullptr;
    double *eta = nullptr, *delta = nullptr, *omega = nullptr;
    double *obj_omega = nullptr, *obj_delta = nullptr, *obj_top = nullptr;
    long long *obj_face = nullptr;
};
// the estimator over the mesh a system keeps, with the lists *vptr / *vface of the caller (built on first use, as
// csr_error_estimate builds them): fields from V_dev[..][n_cols] and W_dev[n_obj][n_cols]
int csr_goal_error(padne_ctx *ctx, const padne_csr *L, int **vptr, int **vface, int n_cols, int n_obj, const double *W_dev,
                   const double *V_dev, const GoalOut &out, int *bad_dev);

}  // namespace padne
