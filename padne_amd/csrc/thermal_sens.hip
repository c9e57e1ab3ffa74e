// Temperature sensitivities by adjoints ("Temperature sensitivities").  No reference counterpart.
//
// After the electrical block M x_c = r_c of the load cases and the thermal block A theta_c = b(x_c), an objective j of case
// c = case[j] is T_j = ambient + g_j^T theta_c.  With x = x_c, theta = theta_c and the corners (1, 2, 3) of a face in the
// order of error_corners, its weights w_12, w_23, w_31 = cot_half of the opposite corner:
//
//   g_j        kind 0, a point: the sampler's weights o_k / s, s = (o_a + o_b) + o_c, at the corners of the owner face (the
//              containing face of the layer with the lowest global number, locate.hpp's sides); kind 1, listed (unknown,
//              weight) pairs; kind 2, source s: g_v = the sum over the faces f of v's list, front to back, that s loads of
//              (area_f / A_s) / 3 -- the load of sources.hip with unit power;
//   lambda_j   A lambda_j = g_j, all objectives in one padne_solve_spd_dev on the hierarchy the forward solve built;
//   lbar_f     = ((lambda_1 + lambda_2) + lambda_3) / 3, the face mean of padne_thermal_report;
//   c_j[i]     = the sum over the faces f of vertex i's list, front to back, of (2 lbar_f) * (sigma * d), d = w_ik (x_i -
//              x_k) + w_il (x_i - x_l) over the two edges of f at i in the order (12, 23, 31); then, with element heat, per
//              resistor (a, b, R) in list order t = (2 ((lambda_a + lambda_b) / 2)) * ((x_a - x_b) / R), +t at a and -t
//              at b; 0 on every row that is no potential.  The block [N][n_obj] row-major, the layout of the plan's r;
//   mu_j       M^T mu_j = c_j: padne_kkt_solve_block_dev and padne_kkt_finish_block on the plan (M is symmetric here);
//   e_j,f      = lbar_f P_f + sigma ((w_12 (mu_1 - mu_2) (x_1 - x_2) + w_23 ...) + w_31 ...),  P_f = face_edge_power
//   k_j,f      = -(kappa ((w_12 (lambda_1 - lambda_2) (theta_1 - theta_2) + w_23 ...) + w_31 ...))
//   film_j,m   = the sum over the vertices v of mesh m of -((hM_v lambda_v) theta_v)
//   pair_j,p   = -(the sum over the vertices i of layer a and their stored partners k in layer b, ascending, of
//              (-G_ik) ((lambda_i - lambda_k) (theta_i - theta_k))), the order of padne_thermal_stack_flows
//   source_j,s = padne_thermal_source_report's sum with lambda_j in the place of theta.
//
// Every kernel is a gather or a stream bound by memory: one thread per vertex, face or unknown in workgroups of 256, the
// per-objective fields field-major ([objective][unknown], [objective][face]) so a wave reads and writes neighbouring
// doubles; the objectives go in register chunks so that a face's corners, coordinates and weights are read once per chunk.
// No floating-point atomics; the sums go through the fixed-order reductions of error.hpp: two calls give the same bits.
// Compiled with -ffp-contract=off: the expressions round as written.
#include "locate.hpp"
#include "thermal.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

struct padne_tsens {
    padne_ctx *ctx = nullptr;
    padne_thermal *th = nullptr;             // borrowed
    padne_kkt *plan = nullptr;               // borrowed
    long long n_pot = 0, N = 0;
    int n_case = 0, n_obj = 0;
    double *kappa = nullptr;                 // [n_mesh] on the device
    double *x = nullptr, *theta = nullptr;   // [n_case][n_pot] copies of what the later solves overwrite
    double *lam = nullptr;                   // [n_obj][n_pot]
    double *rhs = nullptr;                   // [N][n_obj] the electrical adjoints' right-hand sides
    int *obj_case = nullptr;                 // [n_obj] on the device
    bool have_lam = false, have_rhs = false;
};

namespace padne {

constexpr int kTsensChunk = 4;         // objectives per register chunk of the gather and face kernels (fields.hip's 4)
constexpr int kTsensMaxObjectives = 4096;

// x[c][i] = V[i][c] for the potentials i < n_pot of the finished block V[N][n_cols]
__global__ __launch_bounds__(256) void tsens_take_kernel(const long long n_pot, const int n_cols, const double *__restrict__ V,
                                                         double *__restrict__ x) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    for (int c = 0; c < n_cols; ++c) x[(long long)c * n_pot + i] = V[i * n_cols + c];
}

// Objective j = blockIdx.x of kind 0: the owner of its point among the faces of its layer, looked for among all of them (the
// rule of locate_owner), and the sampler's weights at its corners: unknown[3 j + k] = tri[f][k], weight[3 j + k] = o_k / s;
// unknown -1 for a point on no face.  Other kinds are left as the host wrote them
__global__ __launch_bounds__(256) void tsens_owner_kernel(const int n_mesh, const int *__restrict__ mesh_layer,
                                                          const long long *__restrict__ toff, const long long *__restrict__ voff,
                                                          const int32_t *__restrict__ tri, const double *__restrict__ xy,
                                                          const int *__restrict__ kind, const int *__restrict__ arg,
                                                          const double *__restrict__ q, long long *__restrict__ unknown,
                                                          double *__restrict__ weight) {
    __shared__ int red[4];
    const int j = blockIdx.x;
    if (kind[j] != 0) return;                                // (the same for the whole workgroup)
    const int layer = arg[j];
    const double qx = q[2 * j], qy = q[2 * j + 1];
    int best = kNoOwner;
    for (int m = 0; m < n_mesh; ++m) {
        if (mesh_layer[m] != layer) continue;
        const long long v0 = voff[m], nv = voff[m + 1] - v0;
        for (long long t = toff[m] + threadIdx.x; t < toff[m + 1]; t += 256) {
            const int la = tri[3 * t], lb = tri[3 * t + 1], lc = tri[3 * t + 2];
            if (la < 0 || lb < 0 || lc < 0 || la >= nv || lb >= nv || lc >= nv) continue;
            const int a = (int)(v0 + la), b = (int)(v0 + lb), c = (int)(v0 + lc);
            const double xa = xy[2 * (long long)a], ya = xy[2 * (long long)a + 1];
            const double xb = xy[2 * (long long)b], yb = xy[2 * (long long)b + 1];
            const double xc = xy[2 * (long long)c], yc = xy[2 * (long long)c + 1];
            const double oa = edge_side(b, c, xb, yb, xc, yc, qx, qy);
            const double ob = edge_side(c, a, xc, yc, xa, ya, qx, qy);
            const double oc = edge_side(a, b, xa, ya, xb, yb, qx, qy);
            const bool in = ((oa >= 0.0 && ob >= 0.0 && oc >= 0.0) || (oa <= 0.0 && ob <= 0.0 && oc <= 0.0)) &&
                            !(oa == 0.0 && ob == 0.0 && oc == 0.0);
            if (in && (int)t < best) best = (int)t;
        }
    }
    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_down(best, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    best = min(min(red[0], red[1]), min(red[2], red[3]));
    if (best == kNoOwner) {
        for (int k = 0; k < 3; ++k) {
            unknown[3 * j + k] = -1;
            weight[3 * j + k] = 0.0;
        }
        return;
    }
    const long long t = best;
    const long long v0 = voff[find_segment(toff, n_mesh, t)];
    const int a = (int)(v0 + tri[3 * t]), b = (int)(v0 + tri[3 * t + 1]), c = (int)(v0 + tri[3 * t + 2]);
    const double xa = xy[2 * (long long)a], ya = xy[2 * (long long)a + 1];
    const double xb = xy[2 * (long long)b], yb = xy[2 * (long long)b + 1];
    const double xc = xy[2 * (long long)c], yc = xy[2 * (long long)c + 1];
    const double oa = edge_side(b, c, xb, yb, xc, yc, qx, qy);
    const double ob = edge_side(c, a, xc, yc, xa, ya, qx, qy);
    const double oc = edge_side(a, b, xa, ya, xb, yb, qx, qy);
    const double s = (oa + ob) + oc;
    unknown[3 * j] = a;
    unknown[3 * j + 1] = b;
    unknown[3 * j + 2] = c;
    weight[3 * j] = oa / s;
    weight[3 * j + 1] = ob / s;
    weight[3 * j + 2] = oc / s;
}

// g[q][i] of the nq <= kThermalChunk objectives that start at j0.  One thread per unknown; `walk`: an objective of the chunk
// is a source, so the vertices walk their lists (once for the whole chunk) like sources_load_kernel
__global__ __launch_bounds__(256) void tsens_g_kernel(const long long n_pot, const long long n_vert, const int j0, const int nq,
                                                      const int *__restrict__ kind, const int *__restrict__ arg,
                                                      const long long *__restrict__ unknown, const double *__restrict__ weight,
                                                      const bool walk, const int *__restrict__ vptr, const int *__restrict__ vface,
                                                      const double *__restrict__ area, const int *__restrict__ fptr,
                                                      const int *__restrict__ fsrc, const double *__restrict__ A,
                                                      double *__restrict__ g) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    double acc[kThermalChunk];
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q) acc[q] = 0.0;
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q)
        if (q < nq && kind[j0 + q] != 2)
            for (int k = 0; k < 3; ++k)
                if (unknown[3 * (j0 + q) + k] == i) acc[q] = acc[q] + weight[3 * (j0 + q) + k];
    if (walk && i < n_vert)
        for (int e = vptr[i], e1 = vptr[i + 1]; e < e1; ++e) {
            const long long f = vface[e];
            const int k1 = fptr[f + 1];
            if (fptr[f] == k1) continue;
            const double af = area[f];
            for (int k = fptr[f]; k < k1; ++k) {
                const int s = fsrc[k];
                const double third = (af / A[s]) / 3;
#pragma unroll
                for (int q = 0; q < kThermalChunk; ++q)
                    if (q < nq && kind[j0 + q] == 2 && arg[j0 + q] == s) acc[q] = acc[q] + third;
            }
        }
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q)
        if (q < nq) g[(long long)(j0 + q) * n_pot + i] = acc[q];
}

// out[j][p] = field[j][probe[p]]
__global__ __launch_bounds__(256) void tsens_probe_kernel(const int n_probe, const long long n_pot, const long long *__restrict__ probe,
                                                          const double *__restrict__ field, double *__restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_probe) return;
    out[(long long)blockIdx.y * n_probe + p] = field[(long long)blockIdx.y * n_pot + probe[p]];
}

// The copper part of c_j for the nq <= kTsensChunk objectives that start at j0, into rhs[N][n_obj].  One thread per unknown
// walks its list of faces front to back; a face's corners, coordinates and weights are read once for the chunk, every
// objective reads lambda_j and the x of its own case
__global__ __launch_bounds__(256) void tsens_rhs_kernel(const long long N, const long long n_pot, const long long n_vert,
                                                        const int n_mesh, const int32_t *__restrict__ tri,
                                                        const double *__restrict__ xy, const long long *__restrict__ voff,
                                                        const long long *__restrict__ toff, const double *__restrict__ sigma,
                                                        const int *__restrict__ vptr, const int *__restrict__ vface,
                                                        const int n_obj, const int j0, const int nq,
                                                        const int *__restrict__ obj_case, const double *__restrict__ lam,
                                                        const double *__restrict__ x, double *__restrict__ rhs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double acc[kTsensChunk];
    const double *lj[kTsensChunk], *xj[kTsensChunk];
#pragma unroll
    for (int q = 0; q < kTsensChunk; ++q) {
        acc[q] = 0.0;
        const int j = q < nq ? j0 + q : j0;
        lj[q] = lam + (long long)j * n_pot;
        xj[q] = x + (long long)obj_case[j] * n_pot;
    }
    if (i < n_vert)
        for (int e = vptr[i], e1 = vptr[i + 1]; e < e1; ++e) {
            const long long t = vface[e];
            const int m = find_segment(toff, n_mesh, t);
            long long g1, g2, g3;
            if (!error_corners(tri, voff, m, t, g1, g2, g3)) continue;      // (refused when the lists were built)
            const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
            const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
            const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
            const double w23 = cot_half(x2, y2, x3, y3, x1, y1);
            const double w31 = cot_half(x3, y3, x1, y1, x2, y2);
            const double w12 = cot_half(x1, y1, x2, y2, x3, y3);
            const double s = sigma[m];
#pragma unroll
            for (int q = 0; q < kTsensChunk; ++q)
                if (q < nq) {
                    const double lbar = ((lj[q][g1] + lj[q][g2]) + lj[q][g3]) / 3;
                    const double f1 = xj[q][g1], f2 = xj[q][g2], f3 = xj[q][g3];
                    double d;
                    if (i == g1) d = w12 * (f1 - f2) + w31 * (f1 - f3);
                    else if (i == g2) d = w12 * (f2 - f1) + w23 * (f2 - f3);
                    else d = w23 * (f3 - f2) + w31 * (f3 - f1);
                    acc[q] = acc[q] + (2 * lbar) * (s * d);
                }
        }
#pragma unroll
    for (int q = 0; q < kTsensChunk; ++q)
        if (q < nq) rhs[i * n_obj + (j0 + q)] = acc[q];
}

// The resistors' part of c_j: the entries (resistor, sign) grouped by the unknown they add into, their list order kept inside
// a group; one thread per (group, objective j = blockIdx.y) adds its own in that order, like thermal_heat_kernel
__global__ __launch_bounds__(256) void tsens_rhs_res_kernel(const int n_groups, const int *__restrict__ group_ptr,
                                                            const long long *__restrict__ group_dst, const int *__restrict__ entry_res,
                                                            const double *__restrict__ entry_sign, const long long *__restrict__ res_a,
                                                            const long long *__restrict__ res_b, const double *__restrict__ res_R,
                                                            const long long n_pot, const int n_obj, const int *__restrict__ obj_case,
                                                            const double *__restrict__ lam, const double *__restrict__ x,
                                                            double *__restrict__ rhs) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const int j = blockIdx.y;
    const double *l = lam + (long long)j * n_pot, *xc = x + (long long)obj_case[j] * n_pot;
    const long long at = group_dst[g] * n_obj + j;
    double a = rhs[at];
    for (int e = group_ptr[g], e1 = group_ptr[g + 1]; e < e1; ++e) {
        const int r = entry_res[e];
        const long long ia = res_a[r], ib = res_b[r];
        const double t = (2 * ((l[ia] + l[ib]) / 2)) * ((xc[ia] - xc[ib]) / res_R[r]);
        a = a + entry_sign[e] * t;
    }
    rhs[at] = a;
}

// Per face of a tile (256 faces of one mesh, the layout of sensitivity_block_kernel) and objective j: e_out, k_out, c_out
// [j][t] = e / area, k / area and (e + k) / area, and per tile the sums of e and of k in the fixed order of error.hpp.  mu is
// the finished block [N][n_obj] of the electrical adjoints
__global__ __launch_bounds__(256) void tsens_face_kernel(const int n_mesh, const long long *__restrict__ tile_off,
                                                         const int32_t *__restrict__ tri, const double *__restrict__ xy,
                                                         const long long *__restrict__ voff, const long long *__restrict__ toff,
                                                         const double *__restrict__ sigma, const double *__restrict__ kappa,
                                                         const long long n_tri, const long long n_pot, const long long n_blocks,
                                                         const int n_obj, const int *__restrict__ obj_case,
                                                         const double *__restrict__ lam, const double *__restrict__ theta,
                                                         const double *__restrict__ x, const double *__restrict__ mu,
                                                         double *__restrict__ e_out, double *__restrict__ k_out,
                                                         double *__restrict__ c_out, double *__restrict__ tile_e,
                                                         double *__restrict__ tile_k) {
    __shared__ double red_e[kTsensChunk][4], red_k[kTsensChunk][4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    long long g1 = 0, g2 = 0, g3 = 0;
    const bool live = t < toff[m + 1] && error_corners(tri, voff, m, t, g1, g2, g3);
    double w12 = 0, w23 = 0, w31 = 0, area = 1, s = 0, kap = 0;
    if (live) {
        const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
        const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
        const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
        w23 = cot_half(x2, y2, x3, y3, x1, y1);
        w31 = cot_half(x3, y3, x1, y1, x2, y2);
        w12 = cot_half(x1, y1, x2, y2, x3, y3);
        area = error_area(x1, y1, x2, y2, x3, y3);
        s = sigma[m];
        kap = kappa[m];
    }
    const double *m1 = mu + g1 * n_obj, *m2 = mu + g2 * n_obj, *m3 = mu + g3 * n_obj;
    for (int j0 = 0; j0 < n_obj; j0 += kTsensChunk) {
#pragma unroll
        for (int q = 0; q < kTsensChunk; ++q) {
            const int j = j0 + q;
            double ef = 0.0, kf = 0.0;
            if (live && j < n_obj) {
                const double *l = lam + (long long)j * n_pot;
                const long long c = obj_case[j];
                const double *th = theta + c * n_pot, *xc = x + c * n_pot;
                const double l1 = l[g1], l2 = l[g2], l3 = l[g3];
                const double t1 = th[g1], t2 = th[g2], t3 = th[g3];
                const double f1 = xc[g1], f2 = xc[g2], f3 = xc[g3];
                const double u1 = m1[j], u2 = m2[j], u3 = m3[j];
                const double lbar = ((l1 + l2) + l3) / 3;
                ef = lbar * face_edge_power(s, w12, w23, w31, f1, f2, f3) +
                     s * ((w12 * (u1 - u2) * (f1 - f2) + w23 * (u2 - u3) * (f2 - f3)) + w31 * (u3 - u1) * (f3 - f1));
                kf = -(kap * ((w12 * (l1 - l2) * (t1 - t2) + w23 * (l2 - l3) * (t2 - t3)) + w31 * (l3 - l1) * (t3 - t1)));
                const long long at = (long long)j * n_tri + t;
                e_out[at] = ef / area;
                k_out[at] = kf / area;
                c_out[at] = (ef + kf) / area;
            }
            ef = error_wave_sum(ef);
            kf = error_wave_sum(kf);
            if ((threadIdx.x & 63) == 0) {
                red_e[q][threadIdx.x >> 6] = ef;
                red_k[q][threadIdx.x >> 6] = kf;
            }
        }
        __syncthreads();
        if (threadIdx.x < kTsensChunk && j0 + (int)threadIdx.x < n_obj) {
            const int q = threadIdx.x;
            tile_e[(long long)(j0 + q) * n_blocks + b] = error_sum4(red_e[q]);
            tile_k[(long long)(j0 + q) * n_blocks + b] = error_sum4(red_k[q]);
        }
        __syncthreads();
    }
}

// Per tile (256 vertices of one mesh, the layout of thermal_report_vertex_kernel) and objective j: tile[j][b] = the sum of
// -((hM[v] lambda_j[v]) theta_c[v]) in the fixed order of error.hpp
__global__ __launch_bounds__(256) void tsens_vertex_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                           const long long *__restrict__ voff, const long long n_pot,
                                                           const long long n_blocks, const int n_obj,
                                                           const int *__restrict__ obj_case, const double *__restrict__ hM,
                                                           const double *__restrict__ lam, const double *__restrict__ theta,
                                                           double *__restrict__ tile) {
    __shared__ double red[4];
    const long long b = blockIdx.x;
    const int m = find_segment(vtile_off, n_mesh, b);
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    const bool live = v < voff[m + 1];
    const double hm = live ? hM[v] : 0.0;
    for (int j = 0; j < n_obj; ++j) {
        double a = 0.0;
        if (live) a = -((hm * lam[(long long)j * n_pot + v]) * theta[(long long)obj_case[j] * n_pot + v]);
        a = error_wave_sum(a);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x == 0) tile[(long long)j * n_blocks + b] = error_sum4(red);
        __syncthreads();
    }
}

// Per tile of vertices, pair p and objective j, in stack_flow_kernel's order: tile[(j n_pair + p)][b] = the sum over the tile's
// vertices i of a mesh of layer pair_a[p] and their partners k in layer pair_b[p], ascending, of (-G_ik) ((lambda_i - lambda_k)
// (theta_i - theta_k)); 0 for the tiles of other layers
__global__ __launch_bounds__(256) void tsens_pair_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                         const long long *__restrict__ voff, const long long n_pot,
                                                         const long long n_blocks, const int n_obj, const int *__restrict__ obj_case,
                                                         const int n_pair, const int *__restrict__ pair_a,
                                                         const int *__restrict__ pair_b, const int *__restrict__ mesh_layer,
                                                         const int *__restrict__ vertex_layer, const int *__restrict__ gptr,
                                                         const int *__restrict__ gcol, const double *__restrict__ gval,
                                                         const double *__restrict__ lam, const double *__restrict__ theta,
                                                         double *__restrict__ tile) {
    __shared__ double red[4];
    const long long b = blockIdx.x;
    const int m = find_segment(vtile_off, n_mesh, b);
    const long long v = voff[m] + (b - vtile_off[m]) * 256 + threadIdx.x;
    const bool live = v < voff[m + 1];
    const int la = mesh_layer[m];
    const int e0 = live ? gptr[v] : 0, e1 = live ? gptr[v + 1] : 0;
    for (int p = 0; p < n_pair; ++p) {
        const bool mine = pair_a[p] == la;          // (the same for the whole workgroup)
        const int lb = pair_b[p];
        for (int j = 0; j < n_obj; ++j) {
            double acc = 0.0;
            if (mine && live) {
                const double *l = lam + (long long)j * n_pot, *th = theta + (long long)obj_case[j] * n_pot;
                const double li = l[v], ti = th[v];
                for (int e = e0; e < e1; ++e) {
                    const long long k = gcol[e];
                    if (vertex_layer[k] != lb) continue;
                    acc = acc + (-gval[e]) * ((li - l[k]) * (ti - th[k]));
                }
            }
            acc = error_wave_sum(acc);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) tile[((long long)j * n_pair + p) * n_blocks + b] = error_sum4(red);
            __syncthreads();
        }
    }
}

// out[y][m] = the sum of tile[y][..] over the tiles of mesh m = blockIdx.x, y = blockIdx.y: strided partial sums, then the
// wave and workgroup order of error.hpp
__global__ __launch_bounds__(256) void tsens_fold_kernel(const int n_mesh, const long long n_blocks,
                                                         const long long *__restrict__ tile_off, const double *__restrict__ tile,
                                                         double *__restrict__ out) {
    __shared__ double red[4];
    const int m = blockIdx.x;
    const long long at = (long long)blockIdx.y * n_blocks;
    double s = 0.0;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) s += tile[at + i];
    s = error_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(long long)blockIdx.y * n_mesh + m] = error_sum4(red);
}

static void tsens_free(padne_tsens *ts) {
    if (ts == nullptr) return;
    padne_ctx *ctx = ts->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)ts->kappa, (void *)ts->x, (void *)ts->theta, (void *)ts->lam, (void *)ts->rhs, (void *)ts->obj_case})
        if (p != nullptr) pool_free(ctx, p);
    delete ts;
}

static int tsens_require(const char *entry, padne_ctx *ctx, const padne_tsens *ts) {
    PADNE_REQUIRE(ctx && ts, "null argument");
    PADNE_REQUIRE(ts->ctx == ctx, (std::string(entry) + ": the handle belongs to another context").c_str());
    return PADNE_OK;
}

template <typename T> static int tsens_upload(padne_ctx *ctx, Scratch &sc, T **out, const T *host, size_t count) {
    PADNE_TRY(sc.alloc(out, count));
    if (count > 0) PADNE_HIP_CHECK(hipMemcpyAsync(*out, host, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
    return PADNE_OK;
}

// the per-mesh sums of tile[ny][n_blocks] home: out_host[ny][n_mesh]
static int tsens_fold(padne_ctx *ctx, int n_mesh, long long n_blocks, const long long *d_tile_off, const double *d_tile, size_t ny,
                      double *out_host) {
    PADNE_REQUIRE(ny <= 65535, "too many objectives (times pairs) for one launch");
    Scratch sc(ctx);
    double *d_out = nullptr;
    PADNE_TRY(sc.alloc(&d_out, ny * (size_t)n_mesh));
    hipLaunchKernelGGL(tsens_fold_kernel, dim3((unsigned)n_mesh, (unsigned)ny), dim3(256), 0, ctx->stream, n_mesh, n_blocks, d_tile_off,
                       d_tile, d_out);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, sizeof(double) * ny * (size_t)n_mesh, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_tsens_create(padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cases, int32_t n_mesh,
                                  const double *kappa, padne_tsens **out) {
    PADNE_REQUIRE(out && kappa, "null argument");
    PADNE_REQUIRE(n_cases >= 1 && n_cases <= 4096, "between 1 and 4096 load cases");
    const double *V = nullptr;
    PADNE_TRY(thermal_kkt_block("padne_tsens_create", ctx, th, plan, n_cases, &V));
    PADNE_REQUIRE(th->film == nullptr, "a thermal handle with film curves takes no sensitivity handle: the adjoint reads A and hM as constants");
    PADNE_REQUIRE(th->solved && th->n_cols == n_cases, "padne_tsens_create follows a thermal solve of as many columns");
    PADNE_REQUIRE(n_mesh == th->n_mesh, "n_mesh must be that of the system's mesh");
    for (int m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(std::isfinite(kappa[m]) && kappa[m] > 0.0, "the thermal sheet conductance of every mesh must be finite and positive");
    long long N = 0;
    const padne_csr *L = nullptr;
    PADNE_TRY(kkt_finished_block("padne_tsens_create", ctx, plan, n_cases, &V, &N, &L));
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_tsens *ts = new padne_tsens;
    struct Guard {
        padne_tsens *ts;
        ~Guard() { tsens_free(ts); }
    } guard{ts};
    ts->ctx = ctx;
    ts->th = th;
    ts->plan = plan;
    ts->n_pot = th->n_pot;
    ts->N = N;
    ts->n_case = n_cases;
    const size_t count = (size_t)n_cases * (size_t)(th->n_pot > 0 ? th->n_pot : 1);
    ts->kappa = (double *)pool_alloc(ctx, sizeof(double) * (size_t)(n_mesh > 0 ? n_mesh : 1));
    ts->x = (double *)pool_alloc(ctx, sizeof(double) * count);
    ts->theta = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (!ts->kappa || !ts->x || !ts->theta) return PADNE_E_NOMEM;
    PADNE_HIP_CHECK(hipMemcpyAsync(ts->kappa, kappa, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    if (th->n_pot > 0) {
        hipLaunchKernelGGL(tsens_take_kernel, dim3(nblk(th->n_pot)), dim3(256), 0, s, th->n_pot, (int)n_cases, V, ts->x);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(ts->theta, th->theta, sizeof(double) * (size_t)n_cases * (size_t)th->n_pot, hipMemcpyDeviceToDevice, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    guard.ts = nullptr;
    *out = ts;
    return PADNE_OK;
}

extern "C" int padne_tsens_destroy(padne_tsens *ts) {
    tsens_free(ts);
    return PADNE_OK;
}

extern "C" int padne_tsens_thermal_adjoints(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, const int32_t *obj_case,
                                            const int32_t *obj_kind, const int32_t *obj_arg, const double *obj_xy,
                                            int64_t *obj_unknown, double *obj_weight, int32_t n_mesh, const int32_t *mesh_layer,
                                            int64_t n_probe, const int64_t *probe_idx, double *probe_out,
                                            const padne_solve_opts *opts, padne_solve_info *info) {
    PADNE_TRY(tsens_require("padne_tsens_thermal_adjoints", ctx, ts));
    PADNE_REQUIRE(n_obj >= 1 && n_obj <= kTsensMaxObjectives, "between 1 and 4096 objectives");
    PADNE_REQUIRE(obj_case && obj_kind && obj_arg && obj_xy && obj_unknown && obj_weight, "null argument");
    padne_thermal *th = ts->th;
    PADNE_REQUIRE(n_mesh == th->n_mesh && mesh_layer != nullptr, "n_mesh must be that of the system's mesh, with the layer of every mesh");
    PADNE_REQUIRE(n_probe >= 0 && n_probe <= 0x7fffffffLL && (n_probe == 0 || (probe_idx && probe_out)), "probes");
    for (int64_t p = 0; p < n_probe; ++p) PADNE_REQUIRE(probe_idx[p] >= 0 && probe_idx[p] < ts->n_pot, "probe out of range");
    const padne_sources *sr = th->sources;
    bool walk = false, points = false;
    for (int j = 0; j < n_obj; ++j) {
        PADNE_REQUIRE(obj_case[j] >= 0 && obj_case[j] < ts->n_case, "objective case out of range");
        PADNE_REQUIRE(obj_kind[j] >= 0 && obj_kind[j] <= 2, "objective kind: 0 a point, 1 listed unknowns, 2 a heat source");
        if (obj_kind[j] == 0) {
            PADNE_REQUIRE(std::isfinite(obj_xy[2 * j]) && std::isfinite(obj_xy[2 * j + 1]), "an objective's point must be finite");
            points = true;
        } else if (obj_kind[j] == 1) {
            for (int k = 0; k < 3; ++k) {
                PADNE_REQUIRE(obj_unknown[3 * j + k] >= -1 && obj_unknown[3 * j + k] < ts->n_pot, "objective unknown out of range");
                PADNE_REQUIRE(std::isfinite(obj_weight[3 * j + k]), "objective weights must be finite");
            }
        } else {
            PADNE_REQUIRE(sr != nullptr && obj_arg[j] >= 0 && obj_arg[j] < sr->n_source, "objective heat source out of range");
            walk = true;
        }
    }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const long long n_pot = ts->n_pot;
    const ErrorMesh M = error_mesh_of(th->L);
    ts->have_lam = ts->have_rhs = false;
    if (ts->n_obj != n_obj) {
        for (void **p : {(void **)&ts->lam, (void **)&ts->rhs, (void **)&ts->obj_case}) {
            if (*p != nullptr) pool_free(ctx, *p);
            *p = nullptr;
        }
        ts->n_obj = 0;
        ts->lam = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_obj * (size_t)(n_pot > 0 ? n_pot : 1));
        ts->rhs = (double *)pool_alloc(ctx, sizeof(double) * (size_t)n_obj * (size_t)(ts->N > 0 ? ts->N : 1));
        ts->obj_case = (int *)pool_alloc(ctx, sizeof(int) * (size_t)n_obj);
        if (!ts->lam || !ts->rhs || !ts->obj_case) return PADNE_E_NOMEM;
        ts->n_obj = n_obj;
    }
    Scratch sc(ctx);
    int *d_kind = nullptr, *d_arg = nullptr, *d_layer = nullptr;
    long long *d_unknown = nullptr, *d_probe = nullptr;
    double *d_weight = nullptr, *d_xy = nullptr, *d_g = nullptr, *d_pout = nullptr;
    PADNE_HIP_CHECK(hipMemcpyAsync(ts->obj_case, obj_case, sizeof(int) * (size_t)n_obj, hipMemcpyHostToDevice, s));
    PADNE_TRY(tsens_upload(ctx, sc, &d_kind, (const int *)obj_kind, (size_t)n_obj));
    PADNE_TRY(tsens_upload(ctx, sc, &d_arg, (const int *)obj_arg, (size_t)n_obj));
    PADNE_TRY(tsens_upload(ctx, sc, &d_layer, (const int *)mesh_layer, (size_t)n_mesh));
    PADNE_TRY(tsens_upload(ctx, sc, &d_unknown, (const long long *)obj_unknown, 3 * (size_t)n_obj));
    PADNE_TRY(tsens_upload(ctx, sc, &d_weight, obj_weight, 3 * (size_t)n_obj));
    PADNE_TRY(tsens_upload(ctx, sc, &d_xy, obj_xy, 2 * (size_t)n_obj));
    PADNE_TRY(sc.alloc(&d_g, (size_t)n_obj * (size_t)(n_pot > 0 ? n_pot : 1)));
    if (points) {
        hipLaunchKernelGGL(tsens_owner_kernel, dim3((unsigned)n_obj), dim3(256), 0, s, (int)n_mesh, (const int *)d_layer, M.toff, M.voff,
                           M.tri, M.xy, (const int *)d_kind, (const int *)d_arg, (const double *)d_xy, d_unknown, d_weight);
        PADNE_HIP_CHECK(hipGetLastError());
        // the owners home: the caller's value needs them, and a point on no copper is refused before anything is solved
        PADNE_HIP_CHECK(hipMemcpyAsync(obj_unknown, d_unknown, sizeof(long long) * 3 * (size_t)n_obj, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(obj_weight, d_weight, sizeof(double) * 3 * (size_t)n_obj, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
        for (int j = 0; j < n_obj; ++j)
            if (obj_kind[j] == 0 && obj_unknown[3 * j] < 0) {
                set_error("invalid argument: objective %d: its point lies on no face of the connected meshes of layer %d", j, (int)obj_arg[j]);
                return PADNE_E_INVALID;
            }
    }
    if (n_pot > 0) {
        for (int j0 = 0; j0 < n_obj; j0 += kThermalChunk) {
            const int nq = n_obj - j0 < kThermalChunk ? n_obj - j0 : kThermalChunk;
            hipLaunchKernelGGL(tsens_g_kernel, dim3(nblk(n_pot)), dim3(256), 0, s, n_pot, th->n_vert, j0, nq, (const int *)d_kind,
                               (const int *)d_arg, (const long long *)d_unknown, (const double *)d_weight, walk, (const int *)th->vptr,
                               (const int *)th->vface, (const double *)(sr ? sr->face_area : nullptr), (const int *)(sr ? sr->fptr : nullptr),
                               (const int *)(sr ? sr->fsrc : nullptr), (const double *)(sr ? sr->A : nullptr), d_g);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        PADNE_HIP_CHECK(hipMemsetAsync(ts->lam, 0, sizeof(double) * (size_t)n_obj * (size_t)n_pot, s));
    }
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
    o.flags &= ~(1 | 4);                                // lambda starts from zero, on the hierarchy the forward solve built
    const int rc = padne_solve_spd_dev(ctx, th->A, d_g, ts->lam, n_obj, &o, info);
    if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
    if (n_probe > 0) {
        PADNE_TRY(tsens_upload(ctx, sc, &d_probe, (const long long *)probe_idx, (size_t)n_probe));
        PADNE_TRY(sc.alloc(&d_pout, (size_t)n_obj * (size_t)n_probe));
        hipLaunchKernelGGL(tsens_probe_kernel, dim3(nblk(n_probe), (unsigned)n_obj), dim3(256), 0, s, (int)n_probe, n_pot,
                           (const long long *)d_probe, (const double *)ts->lam, d_pout);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(probe_out, d_pout, sizeof(double) * (size_t)n_obj * (size_t)n_probe, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    ts->have_lam = true;
    return rc;
}

extern "C" int padne_tsens_electrical_rhs(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int64_t n_res, const int64_t *res_a,
                                          const int64_t *res_b, const double *res_R, const void **r_dev_out) {
    PADNE_TRY(tsens_require("padne_tsens_electrical_rhs", ctx, ts));
    PADNE_REQUIRE(ts->have_lam && n_obj == ts->n_obj, "padne_tsens_electrical_rhs follows padne_tsens_thermal_adjoints of as many objectives");
    PADNE_REQUIRE(r_dev_out != nullptr, "null argument");
    PADNE_REQUIRE(n_res >= 0 && n_res <= 0x1fffffffLL && (n_res == 0 || (res_a && res_b && res_R)), "resistors");
    for (int64_t r = 0; r < n_res; ++r) {
        PADNE_REQUIRE(res_a[r] >= 0 && res_a[r] < ts->n_pot && res_b[r] >= 0 && res_b[r] < ts->n_pot, "resistor terminal out of range");
        PADNE_REQUIRE(std::isfinite(res_R[r]) && res_R[r] != 0.0, "a resistance must be finite and not zero");
    }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_thermal *th = ts->th;
    const ErrorMesh M = error_mesh_of(th->L);
    ts->have_rhs = false;
    if (ts->N > 0)
        for (int j0 = 0; j0 < n_obj; j0 += kTsensChunk) {
            const int nq = n_obj - j0 < kTsensChunk ? n_obj - j0 : kTsensChunk;
            hipLaunchKernelGGL(tsens_rhs_kernel, dim3(nblk(ts->N)), dim3(256), 0, s, ts->N, ts->n_pot, th->n_vert, th->n_mesh, M.tri, M.xy,
                               M.voff, M.toff, M.sigma, (const int *)th->vptr, (const int *)th->vface, (int)n_obj, j0, nq,
                               (const int *)ts->obj_case, (const double *)ts->lam, (const double *)ts->x, ts->rhs);
            PADNE_HIP_CHECK(hipGetLastError());
        }
    if (n_res > 0) {
        // the 2 n_res entries (resistor, sign) by the unknown they add into, their list order kept (a stable sort on the host)
        std::vector<int64_t> order(2 * (size_t)n_res);
        std::iota(order.begin(), order.end(), (int64_t)0);
        auto dst = [&](int64_t e) { return (e & 1) ? res_b[e >> 1] : res_a[e >> 1]; };
        std::stable_sort(order.begin(), order.end(), [&](int64_t p, int64_t q) { return dst(p) < dst(q); });
        std::vector<int> group_ptr, entry_res(order.size());
        std::vector<long long> group_dst;
        std::vector<double> entry_sign(order.size());
        for (size_t i = 0; i < order.size(); ++i) {
            const int64_t e = order[i];
            if (i == 0 || dst(e) != group_dst.back()) {
                group_ptr.push_back((int)i);
                group_dst.push_back(dst(e));
            }
            entry_res[i] = (int)(e >> 1);
            entry_sign[i] = (e & 1) ? -1.0 : 1.0;
        }
        group_ptr.push_back((int)order.size());
        const int n_groups = (int)group_dst.size();
        Scratch sc(ctx);
        int *d_ptr = nullptr, *d_res = nullptr;
        long long *d_dst = nullptr, *d_a = nullptr, *d_b = nullptr;
        double *d_sign = nullptr, *d_R = nullptr;
        PADNE_TRY(tsens_upload(ctx, sc, &d_ptr, (const int *)group_ptr.data(), group_ptr.size()));
        PADNE_TRY(tsens_upload(ctx, sc, &d_dst, (const long long *)group_dst.data(), group_dst.size()));
        PADNE_TRY(tsens_upload(ctx, sc, &d_res, (const int *)entry_res.data(), entry_res.size()));
        PADNE_TRY(tsens_upload(ctx, sc, &d_sign, (const double *)entry_sign.data(), entry_sign.size()));
        PADNE_TRY(tsens_upload(ctx, sc, &d_a, (const long long *)res_a, (size_t)n_res));
        PADNE_TRY(tsens_upload(ctx, sc, &d_b, (const long long *)res_b, (size_t)n_res));
        PADNE_TRY(tsens_upload(ctx, sc, &d_R, res_R, (size_t)n_res));
        hipLaunchKernelGGL(tsens_rhs_res_kernel, dim3(nblk(n_groups), (unsigned)n_obj), dim3(256), 0, s, n_groups, (const int *)d_ptr,
                           (const long long *)d_dst, (const int *)d_res, (const double *)d_sign, (const long long *)d_a,
                           (const long long *)d_b, (const double *)d_R, ts->n_pot, (int)n_obj, (const int *)ts->obj_case,
                           (const double *)ts->lam, (const double *)ts->x, ts->rhs);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipStreamSynchronize(s));           // (the copies read the host vectors above before they go)
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    ts->have_rhs = true;
    *r_dev_out = ts->rhs;
    return PADNE_OK;
}

// what the read-outs ask: the thermal adjoints exist for n_obj objectives; *mu_out (unless null) the plan's finished block
// of as many columns, the electrical adjoints
static int tsens_ready(const char *entry, padne_ctx *ctx, const padne_tsens *ts, int32_t n_obj, const double **mu_out) {
    PADNE_TRY(tsens_require(entry, ctx, ts));
    PADNE_REQUIRE(ts->have_lam && n_obj == ts->n_obj,
                  (std::string(entry) + " follows padne_tsens_thermal_adjoints of as many objectives").c_str());
    if (mu_out != nullptr) {
        PADNE_REQUIRE(ts->have_rhs, (std::string(entry) + " follows padne_tsens_electrical_rhs and the block solve of its result").c_str());
        long long N = 0;
        const padne_csr *L = nullptr;
        PADNE_TRY(kkt_finished_block(entry, ctx, ts->plan, n_obj, mu_out, &N, &L));
        PADNE_REQUIRE(N == ts->N && L == ts->th->L, "the plan's finished block is not that of the handle's system");
    }
    return PADNE_OK;
}

extern "C" int padne_tsens_faces(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int64_t n_tri, int32_t n_mesh, double *electrical_out,
                                 double *thermal_out, double *copper_out, double *mesh_electrical_out, double *mesh_thermal_out) {
    const double *mu = nullptr;
    PADNE_TRY(tsens_ready("padne_tsens_faces", ctx, ts, n_obj, &mu));
    padne_thermal *th = ts->th;
    PADNE_REQUIRE(n_tri == th->n_tri && n_mesh == th->n_mesh, "n_tri and n_mesh must be those of the system's mesh");
    PADNE_REQUIRE(mesh_electrical_out && mesh_thermal_out && (n_tri == 0 || (electrical_out && thermal_out && copper_out)), "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const std::vector<long long> ftile = thermal_tiles(th->toff);
    const long long n_fb = ftile[(size_t)n_mesh];
    PADNE_REQUIRE(n_fb <= 0x7fffffffLL, "too many tiles for one launch");
    const ErrorMesh M = error_mesh_of(th->L);
    const size_t no = (size_t)n_obj, nfb = (size_t)(n_fb > 0 ? n_fb : 1), nt = (size_t)(n_tri > 0 ? n_tri : 1);
    Scratch sc(ctx);
    long long *d_ftile = nullptr;
    double *d_e = nullptr, *d_k = nullptr, *d_c = nullptr, *d_tile = nullptr;
    PADNE_TRY(tsens_upload(ctx, sc, &d_ftile, ftile.data(), ftile.size()));
    PADNE_TRY(sc.alloc(&d_e, no * nt));
    PADNE_TRY(sc.alloc(&d_k, no * nt));
    PADNE_TRY(sc.alloc(&d_c, no * nt));
    PADNE_TRY(sc.alloc(&d_tile, 2 * no * nfb));
    if (n_fb > 0) {
        hipLaunchKernelGGL(tsens_face_kernel, dim3((unsigned)n_fb), dim3(256), 0, s, (int)n_mesh, (const long long *)d_ftile, M.tri, M.xy,
                           M.voff, M.toff, M.sigma, (const double *)ts->kappa, (long long)n_tri, ts->n_pot, n_fb, (int)n_obj,
                           (const int *)ts->obj_case, (const double *)ts->lam, (const double *)ts->theta, (const double *)ts->x, mu, d_e,
                           d_k, d_c, d_tile, d_tile + no * nfb);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    std::vector<double> sums(2 * no * (size_t)n_mesh, 0.0);
    PADNE_TRY(tsens_fold(ctx, n_mesh, n_fb, d_ftile, d_tile, 2 * no, sums.data()));
    std::copy(sums.begin(), sums.begin() + (long)(no * (size_t)n_mesh), mesh_electrical_out);
    std::copy(sums.begin() + (long)(no * (size_t)n_mesh), sums.end(), mesh_thermal_out);
    if (n_tri > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(electrical_out, d_e, sizeof(double) * no * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(thermal_out, d_k, sizeof(double) * no * nt, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(copper_out, d_c, sizeof(double) * no * nt, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_tsens_vertices(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_mesh, double *mesh_film_out) {
    PADNE_TRY(tsens_ready("padne_tsens_vertices", ctx, ts, n_obj, nullptr));
    padne_thermal *th = ts->th;
    PADNE_REQUIRE(n_mesh == th->n_mesh, "n_mesh must be that of the system's mesh");
    PADNE_REQUIRE(mesh_film_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const std::vector<long long> vtile = thermal_tiles(th->voff);
    const long long n_vb = vtile[(size_t)n_mesh];
    PADNE_REQUIRE(n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const ErrorMesh M = error_mesh_of(th->L);
    Scratch sc(ctx);
    long long *d_vtile = nullptr;
    double *d_tile = nullptr;
    PADNE_TRY(tsens_upload(ctx, sc, &d_vtile, vtile.data(), vtile.size()));
    PADNE_TRY(sc.alloc(&d_tile, (size_t)n_obj * (size_t)(n_vb > 0 ? n_vb : 1)));
    if (n_vb > 0) {
        hipLaunchKernelGGL(tsens_vertex_kernel, dim3((unsigned)n_vb), dim3(256), 0, s, (int)n_mesh, (const long long *)d_vtile, M.voff,
                           ts->n_pot, n_vb, (int)n_obj, (const int *)ts->obj_case, (const double *)th->hM, (const double *)ts->lam,
                           (const double *)ts->theta, d_tile);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return tsens_fold(ctx, n_mesh, n_vb, d_vtile, d_tile, (size_t)n_obj, mesh_film_out);
}

extern "C" int padne_tsens_pairs(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_pair, double *pair_out) {
    PADNE_TRY(tsens_ready("padne_tsens_pairs", ctx, ts, n_obj, nullptr));
    padne_thermal *th = ts->th;
    const padne_stack *st = th->stack;
    PADNE_REQUIRE(n_pair == (st != nullptr ? st->n_pair : 0), "n_pair must be the pairs of the thermal handle");
    if (n_pair == 0) return PADNE_OK;
    PADNE_REQUIRE(pair_out != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n_mesh = th->n_mesh;
    const std::vector<long long> vtile = thermal_tiles(th->voff);
    const long long n_vb = vtile[(size_t)n_mesh];
    PADNE_REQUIRE(n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const size_t ny = (size_t)n_obj * (size_t)n_pair;
    PADNE_REQUIRE(ny <= 65535, "too many objectives times pairs for one launch");
    const ErrorMesh M = error_mesh_of(th->L);
    std::vector<double> mesh_sum(ny * (size_t)n_mesh, 0.0);
    Scratch sc(ctx);
    long long *d_vtile = nullptr;
    int *d_a = nullptr, *d_b = nullptr;
    double *d_tile = nullptr;
    PADNE_TRY(tsens_upload(ctx, sc, &d_vtile, vtile.data(), vtile.size()));
    PADNE_TRY(tsens_upload(ctx, sc, &d_a, st->pair_a.data(), st->pair_a.size()));
    PADNE_TRY(tsens_upload(ctx, sc, &d_b, st->pair_b.data(), st->pair_b.size()));
    PADNE_TRY(sc.alloc(&d_tile, ny * (size_t)(n_vb > 0 ? n_vb : 1)));
    if (n_vb > 0) {
        hipLaunchKernelGGL(tsens_pair_kernel, dim3((unsigned)n_vb), dim3(256), 0, s, n_mesh, (const long long *)d_vtile, M.voff, ts->n_pot,
                           n_vb, (int)n_obj, (const int *)ts->obj_case, (int)n_pair, (const int *)d_a, (const int *)d_b,
                           (const int *)st->mesh_layer_dev, (const int *)st->vertex_layer, (const int *)st->gptr, (const int *)st->gcol,
                           (const double *)st->gval, (const double *)ts->lam, (const double *)ts->theta, d_tile);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_TRY(tsens_fold(ctx, n_mesh, n_vb, d_vtile, d_tile, ny, mesh_sum.data()));
    // the meshes of layer a in ascending order, from 0.0, as padne_thermal_stack_flows joins them; then the sign
    for (int j = 0; j < n_obj; ++j)
        for (int p = 0; p < n_pair; ++p) {
            double sum = 0.0;
            for (int m = 0; m < n_mesh; ++m)
                if (st->mesh_layer[(size_t)m] == st->pair_a[(size_t)p]) sum = sum + mesh_sum[((size_t)j * n_pair + p) * n_mesh + m];
            pair_out[(size_t)j * n_pair + p] = -sum;
        }
    return PADNE_OK;
}

extern "C" int padne_tsens_sources(padne_ctx *ctx, padne_tsens *ts, int32_t n_obj, int32_t n_source, double *source_out) {
    PADNE_TRY(tsens_ready("padne_tsens_sources", ctx, ts, n_obj, nullptr));
    const padne_sources *sr = ts->th->sources;
    PADNE_REQUIRE(n_source == (sr != nullptr ? sr->n_source : 0), "n_source must be the heat sources of the thermal handle");
    if (n_source == 0) return PADNE_OK;
    return sources_report_field(ctx, ts->th, n_obj, ts->lam, source_out);
}
