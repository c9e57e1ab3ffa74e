// The face kernels: what is computed per triangle from solved potentials, on the mesh an assembled system keeps on the
// device or on meshes given by the caller.
//
//   padne_power_density / padne_face_gradient / padne_csr_power_density : sigma |grad V|^2 and grad V of one potential vector
//   launch_power_density_block : the same for every column of a block (padne_kkt_power_density_block)
//   launch_sensitivity_block   : adjoint sensitivities to the conductance of every face (padne_kkt_sensitivity_block)
//   launch_current_faces, launch_current_cuts : J, |J|, hotspots, per-mesh power, the envelope over the columns and the
//                                current through cut segments (padne_kkt_current_report, padne_kkt_current_cases)
//
// Reference arithmetic restated here: compute_triangle_gradient / compute_power_density (solver.py:689-745), with the
// cotangent weights of the assembly (cot_half, face.hpp).  No float atomics: every reduction runs in a fixed order.
//
// This file is compiled with -ffp-contract=off like the assembly: the expressions must round exactly as written.
#include "common.hpp"
#include "face.hpp"

#include <cmath>

namespace padne {


// ---- power density ---------------------------------------------------------------------------
// (interp, face_gradient_of and face_power_of: face.hpp)
__global__ void power_density_kernel(long long n_tri, const int *__restrict__ tri, const double *__restrict__ xy,
                                     int n_mesh, const long long *__restrict__ mesh_voff,
                                     const long long *__restrict__ mesh_toff, const double *__restrict__ sigma,
                                     const double *__restrict__ pot, double *__restrict__ out,
                                     double *__restrict__ gx_out, double *__restrict__ gy_out, int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(mesh_toff, n_mesh, t);
    const long long v0 = mesh_voff[m];
    const long long nv = mesh_voff[m + 1] - v0;
    const int l1 = tri[3 * t + 2], l2 = tri[3 * t], l3 = tri[3 * t + 1];
    if (l1 < 0 || l2 < 0 || l3 < 0 || l1 >= nv || l2 >= nv || l3 >= nv) {      // checked here instead of in a host loop over all triangles
        *(volatile int *)err = 1;
        return;
    }
    const long long g1 = v0 + l1, g2 = v0 + l2, g3 = v0 + l3;
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    const double f1 = pot[g1], f2 = pot[g2], f3 = pot[g3];
    double gx, gy;
    face_gradient_of(x1, y1, x2, y2, x3, y3, f1, f2, f3, gx, gy);
    if (gx_out) {
        gx_out[t] = gx;
        gy_out[t] = gy;
    }
    if (out) out[t] = face_power_of(gx, gy, sigma[m]);
}

// power_density_kernel for a block of n_cols potentials V[n_vert][n_cols] (row-major: the potentials of one vertex in all
// columns are one contiguous run, a 64-byte line for 8 columns) -> out[n_cols][n_tri].  One thread per triangle: the segment
// lookup, the index check and the corners once, then the columns in chunks of kPowerChunk whose loads are in flight together
// (the register count does not grow with n_cols); every column gets the arithmetic of power_density_kernel, hence its bits.
constexpr int kPowerChunk = 8;

__global__ __launch_bounds__(256) void power_density_block_kernel(long long n_tri, const int *__restrict__ tri,
                                                                  const double *__restrict__ xy, int n_mesh,
                                                                  const long long *__restrict__ mesh_voff,
                                                                  const long long *__restrict__ mesh_toff,
                                                                  const double *__restrict__ sigma, const int n_cols,
                                                                  const double *__restrict__ V, double *__restrict__ out,
                                                                  int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(mesh_toff, n_mesh, t);
    const long long v0 = mesh_voff[m];
    const long long nv = mesh_voff[m + 1] - v0;
    const int l1 = tri[3 * t + 2], l2 = tri[3 * t], l3 = tri[3 * t + 1];
    if (l1 < 0 || l2 < 0 || l3 < 0 || l1 >= nv || l2 >= nv || l3 >= nv) {
        *(volatile int *)err = 1;
        return;
    }
    const long long g1 = v0 + l1, g2 = v0 + l2, g3 = v0 + l3;
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    const double s = sigma[m];
    const double *p1 = V + g1 * n_cols, *p2 = V + g2 * n_cols, *p3 = V + g3 * n_cols;
    for (int j0 = 0; j0 < n_cols; j0 += kPowerChunk) {
        double f1[kPowerChunk], f2[kPowerChunk], f3[kPowerChunk];
#pragma unroll
        for (int q = 0; q < kPowerChunk; ++q)
            if (j0 + q < n_cols) {
                f1[q] = p1[j0 + q];
                f2[q] = p2[j0 + q];
                f3[q] = p3[j0 + q];
            }
#pragma unroll
        for (int q = 0; q < kPowerChunk; ++q)
            if (j0 + q < n_cols) {
                double gx, gy;
                face_gradient_of(x1, y1, x2, y2, x3, y3, f1[q], f2[q], f3[q], gx, gy);
                out[(long long)(j0 + q) * n_tri + t] = face_power_of(gx, gy, s);
            }
    }
}

// Adjoint sensitivities of potential differences J_j to the conductance of every face ("Sensitivities").  The
// block V[n_vert..][n_cols] holds x in column 0 and the solutions the adjoints are combined from; adjoint j is
// lambda_j = sum_m W[j][m] V[:, m], formed per corner in registers only.  Per face, with the cot weights of the assembly
// (cot_half, the |cot|/2 of the corner opposite each edge) and the layer's sigma:
//     s_j = sigma * sum_{edges (i,k)} w_ik (lambda_j,i - lambda_j,k) (x_i - x_k)          (= sigma dJ_j / dsigma_face)
// out: power[t] of column 0 with the arithmetic of power_density_kernel (hence its bits), density[j][t] = s_j / area, and
// partial[j][b] = the sum of s_j over block b's faces in a fixed order.  The blocks are tiles of one mesh each (tile_off:
// the first block of every mesh), so the per-mesh totals need no atomics: sensitivity_mesh_fold sums a mesh's tiles.  The
// objectives go in chunks of kSensObjChunk and the columns in chunks of kPowerChunk: registers grow with neither.
constexpr int kSensObjChunk = 4;

__global__ __launch_bounds__(256) void sensitivity_block_kernel(
    int n_mesh, const long long *__restrict__ tile_off, const int *__restrict__ tri, const double *__restrict__ xy,
    const long long *__restrict__ mesh_voff, const long long *__restrict__ mesh_toff, const double *__restrict__ sigma,
    const long long n_tri, const long long n_blocks, const int n_cols, const int n_obj, const double *__restrict__ W,
    const double *__restrict__ V, double *__restrict__ power, double *__restrict__ density, double *__restrict__ partial,
    int *__restrict__ err) {
    __shared__ double red[kSensObjChunk][4];
    const long long b = blockIdx.x;
    const int m = find_segment(tile_off, n_mesh, b);
    const long long t = mesh_toff[m] + (b - tile_off[m]) * 256 + threadIdx.x;
    bool live = t < mesh_toff[m + 1];
    const long long v0 = mesh_voff[m];
    const long long nv = mesh_voff[m + 1] - v0;
    long long g1 = 0, g2 = 0, g3 = 0;
    if (live) {
        const int l1 = tri[3 * t + 2], l2 = tri[3 * t], l3 = tri[3 * t + 1];
        if (l1 < 0 || l2 < 0 || l3 < 0 || l1 >= nv || l2 >= nv || l3 >= nv) {
            *(volatile int *)err = 1;
            live = false;                       // (no return: every thread takes part in the block sums below)
        } else {
            g1 = v0 + l1;
            g2 = v0 + l2;
            g3 = v0 + l3;
        }
    }
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0, u1 = 0, u2 = 0, u3 = 0;
    double w12 = 0, w23 = 0, w31 = 0, area = 1, s = 0;
    const double *p1 = V + g1 * n_cols, *p2 = V + g2 * n_cols, *p3 = V + g3 * n_cols;
    if (live) {
        x1 = xy[2 * g1]; y1 = xy[2 * g1 + 1];
        x2 = xy[2 * g2]; y2 = xy[2 * g2 + 1];
        x3 = xy[2 * g3]; y3 = xy[2 * g3 + 1];
        s = sigma[m];
        u1 = p1[0]; u2 = p2[0]; u3 = p3[0];
        double gx, gy;
        face_gradient_of(x1, y1, x2, y2, x3, y3, u1, u2, u3, gx, gy);
        power[t] = face_power_of(gx, gy, s);
        // the assembly's weights: (tri[0], tri[1], tri[2]) = corners (2, 3, 1) here
        w23 = cot_half(x2, y2, x3, y3, x1, y1);     // edge 2-3, opposite 1
        w31 = cot_half(x3, y3, x1, y1, x2, y2);     // edge 3-1, opposite 2
        w12 = cot_half(x1, y1, x2, y2, x3, y3);     // edge 1-2, opposite 3
        area = fabs((x2 - x1) * (y3 - y1) - (y2 - y1) * (x3 - x1)) / 2;
    }
    const double d12 = u1 - u2, d23 = u2 - u3, d31 = u3 - u1;
    for (int j0 = 0; j0 < n_obj; j0 += kSensObjChunk) {
        double a1[kSensObjChunk], a2[kSensObjChunk], a3[kSensObjChunk];
#pragma unroll
        for (int q = 0; q < kSensObjChunk; ++q) a1[q] = a2[q] = a3[q] = 0.0;
        if (live) {
            for (int c0 = 0; c0 < n_cols; c0 += kPowerChunk) {
                double f1[kPowerChunk], f2[kPowerChunk], f3[kPowerChunk];
#pragma unroll
                for (int c = 0; c < kPowerChunk; ++c)
                    if (c0 + c < n_cols) {
                        f1[c] = p1[c0 + c];
                        f2[c] = p2[c0 + c];
                        f3[c] = p3[c0 + c];
                    }
#pragma unroll
                for (int q = 0; q < kSensObjChunk; ++q)
                    if (j0 + q < n_obj) {
                        const double *w = W + (long long)(j0 + q) * n_cols + c0;
#pragma unroll
                        for (int c = 0; c < kPowerChunk; ++c)
                            if (c0 + c < n_cols) {
                                a1[q] += w[c] * f1[c];
                                a2[q] += w[c] * f2[c];
                                a3[q] += w[c] * f3[c];
                            }
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < kSensObjChunk; ++q) {
            double sj = 0.0;
            if (live && j0 + q < n_obj) {
                sj = s * ((w12 * (a1[q] - a2[q]) * d12 + w23 * (a2[q] - a3[q]) * d23) + w31 * (a3[q] - a1[q]) * d31);
                density[(long long)(j0 + q) * n_tri + t] = sj / area;
            }
            for (int off = 32; off > 0; off >>= 1) sj += __shfl_down(sj, off, 64);
            if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = sj;
        }
        __syncthreads();
        if (threadIdx.x < kSensObjChunk && j0 + (int)threadIdx.x < n_obj) {
            const int q = threadIdx.x;
            partial[(long long)(j0 + q) * n_blocks + b] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        }
        __syncthreads();
    }
}

// total[j][m] = the sum of partial[j][tile_off[m] .. tile_off[m+1]) in a fixed order: one workgroup per (mesh, objective)
__global__ __launch_bounds__(256) void sensitivity_mesh_fold(int n_mesh, const long long *__restrict__ tile_off,
                                                             const long long n_blocks, const double *__restrict__ partial,
                                                             double *__restrict__ total) {
    __shared__ double red[4];
    const int m = blockIdx.x, j = blockIdx.y;
    const double *p = partial + (long long)j * n_blocks;
    double s = 0.0;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) total[(long long)j * n_mesh + m] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Currents ("Currents"): the sheet current density J = -sigma grad V of every face, with the face gradient of
// power_density_kernel (so |J|^2 / sigma is its power density), and the current through cut segments, for the n_report
// leading columns of a block V[g * n_cols + j] in one pass, and the envelope over those columns.  Both kernels run over the
// tile layout of sensitivity_block_kernel: block b is 256 faces of one mesh, its first face below.
__device__ __forceinline__ long long tile_first_face(const long long *__restrict__ tile_off, int n_mesh,
                                                     const long long *__restrict__ mesh_toff, long long b, int &m) {
    m = find_segment(tile_off, n_mesh, b);
    return mesh_toff[m] + (b - tile_off[m]) * 256;
}

// the global corners of face t of mesh m, in the order power_density_kernel visits them; false for an index out of range
__device__ __forceinline__ bool face_corners(const int *__restrict__ tri, const long long *__restrict__ mesh_voff, int m,
                                             long long t, long long &g1, long long &g2, long long &g3) {
    const long long v0 = mesh_voff[m];
    const long long nv = mesh_voff[m + 1] - v0;
    const int l1 = tri[3 * t + 2], l2 = tri[3 * t], l3 = tri[3 * t + 1];
    if (l1 < 0 || l2 < 0 || l3 < 0 || l1 >= nv || l2 >= nv || l3 >= nv) return false;
    g1 = v0 + l1;
    g2 = v0 + l2;
    g3 = v0 + l3;
    return true;
}

// (|J|, face) pairs: the larger |J| wins, the lower face on a tie
__device__ __forceinline__ void hotspot_merge(double &v, long long &f, double ov, long long of) {
    if (ov > v || (ov == v && of < f)) {
        v = ov;
        f = of;
    }
}

constexpr long long kNoFace = 0x7fffffffffffffffLL;

// The corners and xy of a face are read once; the columns go in register chunks of CHUNK (three gathers of 64 contiguous
// bytes each for kCaseChunk), so registers do not grow with n_report.  One reported column takes the instantiation with a
// chunk of 1: the arithmetic of a column does not depend on the chunk, so its bits are the same, and it pays one column's
// reductions and LDS instead of eight.
constexpr int kCaseChunk = 8;

// out, per reported column j: J[j][t][2] and mag[j][t] = |J| (both null: not written), per tile its largest |J| with the face
// (tile_max[j][b], tile_face[j][b]; -1 and kNoFace for no face) and, unless partial is null, partial[j][b] = the tile's sum
// of sigma sum_edges w_ik (V_i - V_k)^2 in the order of sensitivity_block_kernel.  Per face, unless env is null: env[t] =
// max_j |J_j| and env_case[t] the lowest j that attains it (sequential over j: column 0 first, replaced on strictly
// greater only, so a NaN stays with column 0).  Per tile, once: the bounding box of its corners, box[b] = (x_min, y_min,
// x_max, y_max) -- what the host lists cut/tile pairs from.
template <int CHUNK>
__global__ __launch_bounds__(256) void current_cases_face_kernel(
    int n_mesh, const long long *__restrict__ tile_off, const int *__restrict__ tri, const double *__restrict__ xy,
    const long long *__restrict__ mesh_voff, const long long *__restrict__ mesh_toff, const double *__restrict__ sigma,
    const long long n_tri, const long long n_blocks, const int n_cols, const int n_report, const double *__restrict__ V,
    double *__restrict__ J, double *__restrict__ mag, double *__restrict__ env, int *__restrict__ env_case,
    double *__restrict__ tile_max, long long *__restrict__ tile_face, double *__restrict__ partial, double *__restrict__ box,
    int *__restrict__ err) {
    __shared__ double red_v[CHUNK][4], red_p[CHUNK][4], red_box[4][4];
    __shared__ long long red_f[CHUNK][4];
    const long long b = blockIdx.x;
    int m;
    const long long t = tile_first_face(tile_off, n_mesh, mesh_toff, b, m) + threadIdx.x;
    bool live = t < mesh_toff[m + 1];
    long long g1 = 0, g2 = 0, g3 = 0;
    if (live && !face_corners(tri, mesh_voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        live = false;                           // (no return: every thread takes part in the block reductions below)
    }
    const bool fields = J != nullptr, power = partial != nullptr;
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0, w12 = 0, w23 = 0, w31 = 0, s = 0;
    double bx0 = INFINITY, by0 = INFINITY, bx1 = -INFINITY, by1 = -INFINITY;
    if (live) {
        x1 = xy[2 * g1]; y1 = xy[2 * g1 + 1];
        x2 = xy[2 * g2]; y2 = xy[2 * g2 + 1];
        x3 = xy[2 * g3]; y3 = xy[2 * g3 + 1];
        s = sigma[m];
        if (power) {
            w23 = cot_half(x2, y2, x3, y3, x1, y1);     // the weights of sensitivity_block_kernel
            w31 = cot_half(x3, y3, x1, y1, x2, y2);
            w12 = cot_half(x1, y1, x2, y2, x3, y3);
        }
        bx0 = fmin(fmin(x1, x2), x3);
        by0 = fmin(fmin(y1, y2), y3);
        bx1 = fmax(fmax(x1, x2), x3);
        by1 = fmax(fmax(y1, y2), y3);
    }
    for (int off = 32; off > 0; off >>= 1) {
        bx0 = fmin(bx0, __shfl_down(bx0, off, 64));
        by0 = fmin(by0, __shfl_down(by0, off, 64));
        bx1 = fmax(bx1, __shfl_down(bx1, off, 64));
        by1 = fmax(by1, __shfl_down(by1, off, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_box[w][0] = bx0;
        red_box[w][1] = by0;
        red_box[w][2] = bx1;
        red_box[w][3] = by1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) {
            bx0 = fmin(bx0, red_box[q][0]);
            by0 = fmin(by0, red_box[q][1]);
            bx1 = fmax(bx1, red_box[q][2]);
            by1 = fmax(by1, red_box[q][3]);
        }
        box[4 * b] = bx0;
        box[4 * b + 1] = by0;
        box[4 * b + 2] = bx1;
        box[4 * b + 3] = by1;
    }
    const double *p1 = V + g1 * n_cols, *p2 = V + g2 * n_cols, *p3 = V + g3 * n_cols;
    double e = -1.0;
    int ec = 0;
    for (int j0 = 0; j0 < n_report; j0 += CHUNK) {
        double f1[CHUNK], f2[CHUNK], f3[CHUNK];
        if (live) {
#pragma unroll
            for (int q = 0; q < CHUNK; ++q)
                if (j0 + q < n_report) {
                    f1[q] = p1[j0 + q];
                    f2[q] = p2[j0 + q];
                    f3[q] = p3[j0 + q];
                }
        }
#pragma unroll
        for (int q = 0; q < CHUNK; ++q) {
            double a = -1.0, pw = 0.0;
            long long f = kNoFace;
            if (live && j0 + q < n_report) {
                double gx, gy;
                face_gradient_of(x1, y1, x2, y2, x3, y3, f1[q], f2[q], f3[q], gx, gy);
                const double jx = -s * gx, jy = -s * gy;
                a = sqrt(jx * jx + jy * jy);
                f = t;
                if (fields) {
                    const long long at = (long long)(j0 + q) * n_tri + t;
                    J[2 * at] = jx;
                    J[2 * at + 1] = jy;
                    mag[at] = a;
                }
                if (j0 + q == 0 || a > e) {
                    e = a;
                    ec = j0 + q;
                }
                if (power) pw = face_edge_power(s, w12, w23, w31, f1[q], f2[q], f3[q]);
            }
            for (int off = 32; off > 0; off >>= 1) {
                hotspot_merge(a, f, __shfl_down(a, off, 64), __shfl_down(f, off, 64));
                if (power) pw += __shfl_down(pw, off, 64);
            }
            if ((threadIdx.x & 63) == 0) {
                red_v[q][w] = a;
                red_f[q][w] = f;
                red_p[q][w] = pw;
            }
        }
        __syncthreads();
        if (threadIdx.x < CHUNK && j0 + (int)threadIdx.x < n_report) {
            const int q = threadIdx.x;
            double a = red_v[q][0];
            long long f = red_f[q][0];
            for (int r = 1; r < 4; ++r) hotspot_merge(a, f, red_v[q][r], red_f[q][r]);
            const long long at = (long long)(j0 + q) * n_blocks + b;
            tile_max[at] = a;
            tile_face[at] = f;
            if (power) partial[at] = (red_p[q][0] + red_p[q][1]) + (red_p[q][2] + red_p[q][3]);
        }
        __syncthreads();
    }
    if (live && env != nullptr) {
        env[t] = e;
        env_case[t] = ec;
    }
}

// per (mesh m, column j = blockIdx.y), over the mesh's tiles in a fixed order: the largest |J| and its face (global index;
// -1.0 and -1 for a mesh without faces) and, unless partial is null, the power as sensitivity_mesh_fold sums it
__global__ __launch_bounds__(256) void current_cases_mesh_fold(int n_mesh, const long long *__restrict__ tile_off,
                                                               const long long n_blocks, const double *__restrict__ tile_max,
                                                               const long long *__restrict__ tile_face,
                                                               const double *__restrict__ partial, double *__restrict__ mesh_max,
                                                               long long *__restrict__ mesh_face, double *__restrict__ mesh_power) {
    __shared__ double red_v[4], red_p[4];
    __shared__ long long red_f[4];
    const int m = blockIdx.x;
    const long long col = (long long)blockIdx.y * n_blocks;
    const bool power = partial != nullptr;
    double a = -1.0, s = 0.0;
    long long f = kNoFace;
    for (long long i = tile_off[m] + threadIdx.x; i < tile_off[m + 1]; i += 256) {
        hotspot_merge(a, f, tile_max[col + i], tile_face[col + i]);
        if (power) s += partial[col + i];
    }
    for (int off = 32; off > 0; off >>= 1) {
        hotspot_merge(a, f, __shfl_down(a, off, 64), __shfl_down(f, off, 64));
        s += __shfl_down(s, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = a;
        red_f[threadIdx.x >> 6] = f;
        red_p[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) hotspot_merge(a, f, red_v[q], red_f[q]);
        const long long at = (long long)blockIdx.y * n_mesh + m;
        mesh_max[at] = a;
        mesh_face[at] = f == kNoFace ? -1 : f;
        if (power) mesh_power[at] = (red_p[0] + red_p[1]) + (red_p[2] + red_p[3]);
    }
}

// edge (i, k) of a face, cot weight w, against the cut c = (start x, y, end x, y): w (V_left - V_right) when it crosses,
// else 0.  The edge runs from its lower global vertex P to the higher Q, so the two faces of an edge decide alike; it
// crosses when P and Q lie on different sides of the cut's line (on the line counts as right) and start and end on
// different sides of the edge's line
__device__ __forceinline__ double cut_edge(long long gi, long long gk, double xi, double yi, double xk, double yk, double ui,
                                           double uk, double w, const double *c) {
    if (gk < gi) {
        const double tx = xi, ty = yi, tu = ui;
        xi = xk; yi = yk; ui = uk;
        xk = tx; yk = ty; uk = tu;
    }
    const bool lp = orient(c[0], c[1], c[2], c[3], xi, yi) > 0, lq = orient(c[0], c[1], c[2], c[3], xk, yk) > 0;
    if (lp == lq) return 0.0;
    const bool ls = orient(xi, yi, xk, yk, c[0], c[1]) > 0, le = orient(xi, yi, xk, yk, c[2], c[3]) > 0;
    if (ls == le) return 0.0;
    return w * (lp ? ui - uk : uk - ui);
}

// one workgroup per (cut, tile) pair, the n_report leading columns: partial[j][p] = the current of pair p's tile across its
// cut in column j, summed in a fixed order.  The face's share of an edge carries the assembly's weight sigma |cot|/2 of the
// opposite corner (cot_half), so the two faces of an edge together carry the edge's conductance.  sensitivity_mesh_fold
// then sums each (cut, column)'s pairs.
template <int CHUNK>
__global__ __launch_bounds__(256) void current_cases_cut_kernel(
    int n_mesh, const long long *__restrict__ tile_off, const int *__restrict__ tri, const double *__restrict__ xy,
    const long long *__restrict__ mesh_voff, const long long *__restrict__ mesh_toff, const double *__restrict__ sigma,
    const int n_cols, const int n_report, const double *__restrict__ V, const long long n_pairs,
    const int *__restrict__ pair_cut, const long long *__restrict__ pair_tile, const double *__restrict__ cut_xy,
    double *__restrict__ partial, int *__restrict__ err) {
    __shared__ double red[CHUNK][4];
    const long long p = blockIdx.x;
    int m;
    const long long t = tile_first_face(tile_off, n_mesh, mesh_toff, pair_tile[p], m) + threadIdx.x;
    bool live = t < mesh_toff[m + 1];
    long long g1 = 0, g2 = 0, g3 = 0;
    if (live && !face_corners(tri, mesh_voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        live = false;
    }
    const double *c = cut_xy + 4 * (long long)pair_cut[p];
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0, w12 = 0, w23 = 0, w31 = 0, sg = 0;
    if (live) {
        x1 = xy[2 * g1]; y1 = xy[2 * g1 + 1];
        x2 = xy[2 * g2]; y2 = xy[2 * g2 + 1];
        x3 = xy[2 * g3]; y3 = xy[2 * g3 + 1];
        w12 = cot_half(x1, y1, x2, y2, x3, y3);
        w23 = cot_half(x2, y2, x3, y3, x1, y1);
        w31 = cot_half(x3, y3, x1, y1, x2, y2);
        sg = sigma[m];
    }
    const double *p1 = V + g1 * n_cols, *p2 = V + g2 * n_cols, *p3 = V + g3 * n_cols;
    for (int j0 = 0; j0 < n_report; j0 += CHUNK) {
#pragma unroll
        for (int q = 0; q < CHUNK; ++q) {
            double s = 0.0;
            if (live && j0 + q < n_report) {
                const double u1 = p1[j0 + q], u2 = p2[j0 + q], u3 = p3[j0 + q];
                const double e12 = cut_edge(g1, g2, x1, y1, x2, y2, u1, u2, w12, c);
                const double e23 = cut_edge(g2, g3, x2, y2, x3, y3, u2, u3, w23, c);
                const double e31 = cut_edge(g3, g1, x3, y3, x1, y1, u3, u1, w31, c);
                s = sg * ((e12 + e23) + e31);
            }
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s;
        }
        __syncthreads();
        if (threadIdx.x < CHUNK && j0 + (int)threadIdx.x < n_report) {
            const int q = threadIdx.x;
            partial[(long long)(j0 + q) * n_pairs + p] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        }
        __syncthreads();
    }
}
}  // namespace padne

using namespace padne;

// Power density of a solution on the mesh the matrix was assembled from (kept on the device): uploads the potentials,
// downloads one value per triangle.  compute_power_density, solver.py:728-745, for all meshes in one launch.
extern "C" int padne_csr_power_density(padne_ctx *ctx, const padne_csr *m, const double *potential_host,
                                       double *power_out_host) {
    PADNE_REQUIRE(ctx && m, "null argument");
    PADNE_REQUIRE(m->mesh_n_mesh > 0 || m->mesh_n_tri == 0, "the matrix does not carry a mesh (only padne_assemble_system keeps it)");
    if (m->mesh_n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(potential_host && power_out_host, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    double *d_pot = nullptr, *d_out = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_pot, (size_t)m->mesh_n_vert));
    PADNE_TRY(sc.alloc(&d_out, (size_t)m->mesh_n_tri));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_pot, potential_host, sizeof(double) * (size_t)m->mesh_n_vert, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(power_density_kernel, dim3(nblk(m->mesh_n_tri)), dim3(256), 0, s, (long long)m->mesh_n_tri, m->mesh_tri,
                       m->mesh_xy, (int)m->mesh_n_mesh, m->mesh_voff, m->mesh_toff, m->mesh_sigma, d_pot, d_out,
                       (double *)nullptr, (double *)nullptr, d_bad);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(power_out_host, d_out, sizeof(double) * (size_t)m->mesh_n_tri, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

namespace padne {
// power_density_block_kernel over the mesh `m` keeps, for V_dev[mesh_n_vert..][n_cols] (device) -> out_dev[n_cols][mesh_n_tri];
// bad_dev (device int, zeroed by the caller) is set when a triangle names a vertex outside its mesh.  Asynchronous.
int launch_power_density_block(padne_ctx *ctx, const padne_csr *m, int n_cols, const double *V_dev, double *out_dev,
                               int *bad_dev) {
    PADNE_REQUIRE(m->mesh_n_mesh > 0 && m->mesh_xy != nullptr, "the matrix does not carry a mesh (only padne_assemble_system keeps it)");
    if (m->mesh_n_tri == 0 || n_cols == 0) return PADNE_OK;
    hipLaunchKernelGGL(power_density_block_kernel, dim3(nblk(m->mesh_n_tri)), dim3(256), 0, ctx->stream, (long long)m->mesh_n_tri,
                       m->mesh_tri, m->mesh_xy, (int)m->mesh_n_mesh, m->mesh_voff, m->mesh_toff, m->mesh_sigma, n_cols, V_dev,
                       out_dev, bad_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

// sensitivity_block_kernel + sensitivity_mesh_fold over the mesh `m` keeps.  tile_off_host[mesh_n_mesh + 1]: the first
// 256-triangle tile of every mesh (a host array); W_dev[n_obj][n_cols], V_dev[mesh_n_vert..][n_cols], power_dev[mesh_n_tri],
// density_dev[n_obj][mesh_n_tri], total_dev[n_obj][mesh_n_mesh] (device).  Asynchronous; bad_dev as above.
int launch_sensitivity_block(padne_ctx *ctx, const padne_csr *m, const long long *tile_off_host, int n_cols, int n_obj,
                             const double *W_dev, const double *V_dev, double *power_dev, double *density_dev, double *total_dev,
                             int *bad_dev) {
    PADNE_REQUIRE(m->mesh_n_mesh > 0 && m->mesh_xy != nullptr, "the matrix does not carry a mesh (only padne_assemble_system keeps it)");
    const int n_mesh = (int)m->mesh_n_mesh;
    const long long n_blocks = tile_off_host[n_mesh];
    if (n_cols == 0 || n_obj == 0) return PADNE_OK;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    long long *d_tile = nullptr;
    double *d_partial = nullptr;
    PADNE_TRY(sc.alloc(&d_tile, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_partial, (size_t)n_obj * (size_t)(n_blocks > 0 ? n_blocks : 1)));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tile, tile_off_host, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    if (n_blocks > 0) {
        hipLaunchKernelGGL(sensitivity_block_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, n_mesh, (const long long *)d_tile,
                           m->mesh_tri, m->mesh_xy, m->mesh_voff, m->mesh_toff, m->mesh_sigma, (long long)m->mesh_n_tri, n_blocks,
                           n_cols, n_obj, W_dev, V_dev, power_dev, density_dev, d_partial, bad_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sensitivity_mesh_fold, dim3((unsigned)n_mesh, (unsigned)n_obj), dim3(256), 0, s, n_mesh,
                       (const long long *)d_tile, n_blocks, (const double *)d_partial, total_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    // (the scratch goes back to the pool on return: the context's one stream orders its reuse after these launches)
    return PADNE_OK;
}

// current_cases_face_kernel + current_cases_mesh_fold over the mesh `m` keeps, on the tiles tile_dev[mesh_n_mesh + 1]
// (device) of sensitivity_block_kernel's layout, n_blocks of them, for the n_report leading columns of V_dev[..][n_cols]:
// the chunk-1 kernel for one column, else chunks of kCaseChunk.  J_dev[n_report][mesh_n_tri][2] and
// mag_dev[n_report][mesh_n_tri] (both null: no per-column field), env_dev, env_case_dev[mesh_n_tri] (both null: no
// envelope), box_dev[n_blocks][4], mesh_max_dev, mesh_face_dev[n_report][mesh_n_mesh], mesh_power_dev[n_report][mesh_n_mesh]
// (null: no power) (device).  Asynchronous.
int launch_current_faces(padne_ctx *ctx, const padne_csr *m, const long long *tile_dev, long long n_blocks, int n_cols,
                         int n_report, const double *V_dev, double *J_dev, double *mag_dev, double *env_dev, int *env_case_dev,
                         double *box_dev, double *mesh_max_dev, long long *mesh_face_dev, double *mesh_power_dev, int *bad_dev) {
    PADNE_REQUIRE(m->mesh_n_mesh > 0 && m->mesh_xy != nullptr, "the matrix does not carry a mesh (only padne_assemble_system keeps it)");
    PADNE_REQUIRE(n_report >= 1 && n_report <= n_cols && n_report <= 65535, "between 1 and 65535 columns");
    PADNE_REQUIRE((J_dev == nullptr) == (mag_dev == nullptr), "J and |J| go together");
    PADNE_REQUIRE((env_dev == nullptr) == (env_case_dev == nullptr), "the envelope and its cases go together");
    const int n_mesh = (int)m->mesh_n_mesh;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    const size_t nb = (size_t)n_report * (size_t)(n_blocks > 0 ? n_blocks : 1);
    double *d_tmax = nullptr, *d_partial = nullptr;
    long long *d_tface = nullptr;
    PADNE_TRY(sc.alloc(&d_tmax, nb));
    PADNE_TRY(sc.alloc(&d_tface, nb));
    if (mesh_power_dev) PADNE_TRY(sc.alloc(&d_partial, nb));
    if (n_blocks > 0) {
        const auto kernel = n_report == 1 ? current_cases_face_kernel<1> : current_cases_face_kernel<kCaseChunk>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, n_mesh, tile_dev, m->mesh_tri, m->mesh_xy,
                           m->mesh_voff, m->mesh_toff, m->mesh_sigma, (long long)m->mesh_n_tri, n_blocks, n_cols, n_report, V_dev,
                           J_dev, mag_dev, env_dev, env_case_dev, d_tmax, d_tface, d_partial, box_dev, bad_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(current_cases_mesh_fold, dim3((unsigned)n_mesh, (unsigned)n_report), dim3(256), 0, s, n_mesh, tile_dev,
                       n_blocks, (const double *)d_tmax, (const long long *)d_tface, (const double *)d_partial, mesh_max_dev,
                       mesh_face_dev, mesh_power_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    // (the scratch goes back to the pool on return: the context's one stream orders its reuse after these launches)
    return PADNE_OK;
}

// current_cases_cut_kernel over n_pairs (cut, tile) pairs sorted by cut (pair_cut_dev, pair_tile_dev; pair_off_host[n_cut + 1]
// the first pair of every cut, a host array), then each (cut, column)'s pairs summed in a fixed order by
// sensitivity_mesh_fold into cut_dev[n_report][n_cut].  cut_xy_dev[n_cut][4] (device).  Asynchronous.
int launch_current_cuts(padne_ctx *ctx, const padne_csr *m, const long long *tile_dev, int n_cols, int n_report,
                        const double *V_dev, int n_cut, const double *cut_xy_dev, long long n_pairs, const int *pair_cut_dev,
                        const long long *pair_tile_dev, const long long *pair_off_host, double *cut_dev, int *bad_dev) {
    PADNE_REQUIRE(m->mesh_n_mesh > 0 && m->mesh_xy != nullptr, "the matrix does not carry a mesh (only padne_assemble_system keeps it)");
    PADNE_REQUIRE(n_report >= 1 && n_report <= n_cols && n_report <= 65535, "between 1 and 65535 columns");
    if (n_cut == 0) return PADNE_OK;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    long long *d_off = nullptr;
    double *d_partial = nullptr;
    PADNE_TRY(sc.alloc(&d_off, (size_t)n_cut + 1));
    PADNE_TRY(sc.alloc(&d_partial, (size_t)n_report * (size_t)(n_pairs > 0 ? n_pairs : 1)));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_off, pair_off_host, sizeof(long long) * ((size_t)n_cut + 1), hipMemcpyHostToDevice, s));
    if (n_pairs > 0) {
        const auto kernel = n_report == 1 ? current_cases_cut_kernel<1> : current_cases_cut_kernel<kCaseChunk>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, (int)m->mesh_n_mesh, tile_dev, m->mesh_tri, m->mesh_xy,
                           m->mesh_voff, m->mesh_toff, m->mesh_sigma, n_cols, n_report, V_dev, n_pairs, pair_cut_dev,
                           pair_tile_dev, cut_xy_dev, d_partial, bad_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sensitivity_mesh_fold, dim3((unsigned)n_cut, (unsigned)n_report), dim3(256), 0, s, n_cut,
                       (const long long *)d_off, n_pairs, (const double *)d_partial, cut_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}
}  // namespace padne

static int face_fields(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri,
                       const int32_t *tri_host, int64_t n_mesh, const int64_t *mesh_vertex_offset,
                       const int64_t *mesh_tri_offset, const double *conductance, const double *potential_host,
                       double *power_out_host, double *gx_out_host, double *gy_out_host) {
    PADNE_REQUIRE(ctx, "ctx");
    PADNE_REQUIRE(n_vert >= 0 && n_tri >= 0 && n_mesh >= 0, "negative size");
    if (n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(xy_host && tri_host && mesh_vertex_offset && mesh_tri_offset && potential_host && n_mesh > 0,
                  "null argument");
    PADNE_REQUIRE(power_out_host == nullptr || conductance != nullptr, "conductance");
    PADNE_REQUIRE(mesh_vertex_offset[n_mesh] == n_vert && mesh_tri_offset[n_mesh] == n_tri, "offset tables");
    PADNE_REQUIRE(mesh_vertex_offset[0] == 0 && mesh_tri_offset[0] == 0, "offset tables must start at 0");
    for (int64_t m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(mesh_vertex_offset[m] <= mesh_vertex_offset[m + 1] && mesh_tri_offset[m] <= mesh_tri_offset[m + 1],
                      "offset tables not monotone");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    double *d_xy = nullptr, *d_sigma = nullptr, *d_pot = nullptr, *d_out = nullptr, *d_gx = nullptr, *d_gy = nullptr;
    int *d_tri = nullptr, *d_bad = nullptr;
    long long *d_voff = nullptr, *d_toff = nullptr;
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    PADNE_TRY(sc.alloc(&d_xy, (size_t)n_vert * 2));
    PADNE_TRY(sc.alloc(&d_tri, (size_t)n_tri * 3));
    PADNE_TRY(sc.alloc(&d_sigma, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_voff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_toff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_pot, (size_t)n_vert));
    if (power_out_host) PADNE_TRY(sc.alloc(&d_out, (size_t)n_tri));
    if (gx_out_host) {
        PADNE_TRY(sc.alloc(&d_gx, (size_t)n_tri));
        PADNE_TRY(sc.alloc(&d_gy, (size_t)n_tri));
    }
    // (hipMemcpyDefault: the two big arrays may already live on the device -- padne_generate_grid_mesh, padne_assemble_system_ex)
    PADNE_HIP_CHECK(hipMemcpyAsync(d_xy, xy_host, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyDefault, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tri, tri_host, sizeof(int) * 3 * (size_t)n_tri, hipMemcpyDefault, s));
    if (conductance)
        PADNE_HIP_CHECK(hipMemcpyAsync(d_sigma, conductance, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_voff, mesh_vertex_offset, sizeof(long long) * (size_t)(n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_toff, mesh_tri_offset, sizeof(long long) * (size_t)(n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_pot, potential_host, sizeof(double) * (size_t)n_vert, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(power_density_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, (long long)n_tri, d_tri, d_xy, (int)n_mesh,
                       d_voff, d_toff, d_sigma, d_pot, d_out, d_gx, d_gy, d_bad);
    PADNE_HIP_CHECK(hipGetLastError());
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    if (power_out_host)
        PADNE_HIP_CHECK(hipMemcpyAsync(power_out_host, d_out, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, s));
    if (gx_out_host) {
        PADNE_HIP_CHECK(hipMemcpyAsync(gx_out_host, d_gx, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(gy_out_host, d_gy, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}

extern "C" int padne_power_density(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri,
                                   const int32_t *tri_host, int64_t n_mesh, const int64_t *mesh_vertex_offset,
                                   const int64_t *mesh_tri_offset, const double *conductance,
                                   const double *potential_host, double *power_out_host) {
    PADNE_REQUIRE(n_tri == 0 || (power_out_host && conductance), "null argument");
    return face_fields(ctx, n_vert, xy_host, n_tri, tri_host, n_mesh, mesh_vertex_offset, mesh_tri_offset,
                       conductance, potential_host, power_out_host, nullptr, nullptr);
}

extern "C" int padne_face_gradient(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri,
                                   const int32_t *tri_host, int64_t n_mesh, const int64_t *mesh_vertex_offset,
                                   const int64_t *mesh_tri_offset, const double *potential_host,
                                   double *gx_out_host, double *gy_out_host) {
    PADNE_REQUIRE(n_tri == 0 || (gx_out_host && gy_out_host), "null argument");
    return face_fields(ctx, n_vert, xy_host, n_tri, tri_host, n_mesh, mesh_vertex_offset, mesh_tri_offset,
                       nullptr, potential_host, nullptr, gx_out_host, gy_out_host);
}
