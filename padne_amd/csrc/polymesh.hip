// The grid mesher ("Grid mesher"): first meshes of polygons with holes, by isosurface stuffing (Labelle and
// Shewchuk) in two dimensions with every decision made from the unwarped lattice.  Stands where the reference's CGAL mesher
// stands (padne/mesh.py:662-795 -- out of scope); no Delaunay refinement, no exact corners, variable density only as the
// quadtree of "Graded" below.  One call meshes a batch of polygons; polygon p = rings (exterior, holes), a ring = n >= 3
// vertices without a closing duplicate.
//
//   lattice   i0 = floor(xmin / h) - 1, nx = ceil(xmax / h) + 1 - i0 + 1 vertices per row, rows likewise: the bounding box and
//             one cell on every side; x_i = (i0 + i) * h.  Cells split by the diagonal v00-v11 into (v00, v10, v11) and
//             (v00, v11, v01); the edge families E, N, NE start at their lower left vertex A;
//   segments  segment k of a ring runs from vertex k - 1 (cyclic) P = (xj, yj) to vertex k Q = (xi, yi) and belongs to band j
//             (cell row j) when min(yj, yi) <= Y[j + 1] and max(yj, yi) >= Y[j].  The vertices of row j and the edges that
//             start in row j read band j and nothing else: no stage costs segments times vertices;
//   sign      + when the number of segments of the band with (yi > cy) != (yj > cy) and
//             cx < (xj - xi) * (cy - yi) / (yj - yi) + xi is odd (the rule of sources.hip), otherwise -;
//   cut       of an edge A -> B whose ends differ in sign, against P -> Q: r = B - A, s = Q - P, w = P - A,
//             den = rx * sy - ry * sx, t = (wx * sy - wy * sx) / den, u = (wx * ry - wy * rx) / den; it meets when den != 0,
//             0 <= t <= 1 and 0 <= u <= 1; the cut's t is the least such t when A is +, the greatest when B is +, 0.5 when
//             rounding leaves none; the cut lies at A + t * r.  Edges whose ends agree get none;
//   snap      the six directions of a vertex in the order E, N, NE, W, S, SW; the cut of a direction at c,
//             d2 = dx * dx + dy * dy from the vertex to c, l2 = rx * rx + ry * ry of its edge; a candidate when
//             d2 < (snap * snap) * l2; the vertex moves to the candidate of least d2, the lowest direction on a tie, and
//             becomes 0 (on the boundary).  A cut lives while neither of its ends is 0;
//   faces     no + corner: nothing, except three 0 corners whose centroid ((x0 + x1) + x2) / 3 is inside (a polygon side on
//             a lattice line); no - corner: the triangle; one +, two -, + first (p, q, r): (p, cut pq, cut rp); one +, one 0,
//             one -, + first: (p, q, cut rp) or (p, cut pq, r); two +, one -, - last: d1 = |cut qr - p|^2, d2 = |cut rp - q|^2,
//             d1 <= d2: (p, q, cut qr), (p, cut qr, cut rp), otherwise (p, q, cut rp), (q, cut qr, cut rp);
//   numbers   slot v = j * nx + i for a lattice vertex, nv + 3 v + f for the cut of family f that starts at v; the slots some
//             face names are numbered in ascending slot order (lattice vertices row-major, then cuts by vertex and family),
//             faces in cell order, lower triangle first, pieces in the order above: flags, two scans, emit.
//
// Kernels: one workgroup of 256 per (lattice row, 256 vertices of it) for sign and cuts, the band's segments staged through
// LDS 256 at a time (8 KB); everything else one thread per lattice vertex, bound by memory.  The band index is count, scan
// and fill with integer atomics: the order within a band is not fixed and nothing depends on it (parity, least and greatest
// t).  No floating-point atomics; compiled with -ffp-contract=off, so the expressions round as written and
// tests/gridmesh_ref.py reproduces them: two calls give the same bits.
//
// Graded (padne_polymesh_create_graded; DESIGN.md, "Graded grid mesher"; tests/gridmesh_graded_ref.py restates it): steps
// lattice to snap as above, then a balanced quadtree over the cells the boundary does not touch.  Integers only.
//
//   plain     cell (ci, cj), ci < nx - 1, cj < ny - 1, is plain when its four corners have state +; a seed (x, y) makes the
//             cell (floor(x / h) - i0, floor(y / h) - j0) not plain when that cell is in the lattice; cells outside are not plain;
//   distance  d(c) = the Chebyshev distance in cells to the nearest cell that is not plain, capped at t[n_level - 1]: along
//             the row dr = the least k with cell ci - k or ci + k not plain, then d = min over k of max(k, dr of row cj +- k);
//   level     the largest l < n_level such that the block of 2^l x 2^l cells that holds the cell, aligned at global cell
//             indices ((i0 + ci) and (j0 + cj) rounded down to multiples of 2^l), lies in the lattice and min d over it is at
//             least t[l]: a leaf.  t[0] = 0 and t[l] >= t[l - 1] + 2^(l - 1), so leaves that share a side differ by one level
//             at most.  The block minima come level by level from the four blocks below;
//   faces     a level 0 cell as above.  Of a leaf of level l >= 1 the anchor (lower left) cell alone emits, and counts them as
//             its lower triangle's: with the corners v00, v10, v11, v01 of the leaf, a side hangs when the cell across it at the
//             anchor's end (below v00, right of v10, above v01, left of v00) has a lower level; none hangs: (v00, v10, v11),
//             (v00, v11, v01); otherwise with c the lattice vertex at the centre and the ring v00, [mid S], v10, [mid E], v11,
//             [mid N], v01, [mid W], a midpoint on a hanging side only: (c, ring[k], ring[k + 1]) cyclically from v00.
//
// The arrays of the new stages are indexed like the lattice's vertices (cell = its v00; the last row and column hold no cell).
//
// Limits, checked by padne_polymesh_create: a lattice of at most kPolymeshMaxLattice = 2^24 vertices, a batch of at most
// kPolymeshMaxBatch = 2^27 lattice vertices (its 4 slots per vertex, 2 triangles per vertex and 3 cuts per vertex then fit
// int32), fewer than 2^31 entries in the band index.
#include "common.hpp"

#include <cmath>
#include <vector>

namespace padne {

constexpr long long kPolymeshMaxLattice = 1LL << 24;
constexpr long long kPolymeshMaxBatch = 1LL << 27;
constexpr int kPolymeshChunk = 256;       // segments of a band in LDS at a time

struct PolyInfo {       // [n_poly + 1]: the last entry holds the totals in lat_off and row_off
    int lat_off, row_off, nx, ny, i0, j0;
};

__device__ __forceinline__ int polymesh_poly_of_row(const PolyInfo *__restrict__ info, int n_poly, int row) {
    int lo = 0, hi = n_poly - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (info[mid].row_off <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int polymesh_poly_of_vertex(const PolyInfo *__restrict__ info, int n_poly, int gv) {
    int lo = 0, hi = n_poly - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (info[mid].lat_off <= gv) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the even-odd rule over the segments list[0 .. n) of seg (global memory): the three-0 rule's rare test
__device__ __forceinline__ bool polymesh_inside(const double *__restrict__ seg, const int *__restrict__ list, int n, double cx, double cy) {
    bool in = false;
    for (int k = 0; k < n; ++k) {
        const double *s = seg + 4 * (long long)list[k];
        const double xj = s[0], yj = s[1], xi = s[2], yi = s[3];
        if ((yi > cy) != (yj > cy) && cx < (xj - xi) * (cy - yi) / (yj - yi) + xi) in = !in;
    }
    return in;
}

// FILL = false: count[row] = the segments of every band.  FILL = true: band_seg filled from band_ptr[row] on, count the cursor
template <bool FILL>
__global__ __launch_bounds__(256) void polymesh_band_kernel(const int n_seg, const double *__restrict__ seg, const int *__restrict__ seg_poly,
                                                            const PolyInfo *__restrict__ info, const double h, int *count,
                                                            const int *__restrict__ band_ptr, int *__restrict__ band_seg) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg) return;
    const PolyInfo P = info[seg_poly[s]];
    const double y0 = seg[4 * (long long)s + 1], y1 = seg[4 * (long long)s + 3];
    const double ylo = fmin(y0, y1), yhi = fmax(y0, y1);
    // two bands of margin for the rounding of the quotients; the compares below decide
    double a = floor(ylo / h) - (double)P.j0 - 2.0, b = floor(yhi / h) - (double)P.j0 + 2.0;
    a = fmin(fmax(a, 0.0), (double)(P.ny - 1));
    b = fmin(fmax(b, 0.0), (double)(P.ny - 1));
    for (int j = (int)a; j <= (int)b; ++j) {
        const double Yj = (double)(P.j0 + j) * h, Yj1 = (double)(P.j0 + j + 1) * h;
        if (ylo <= Yj1 && yhi >= Yj) {
            const int at = atomicAdd(count + P.row_off + j, 1);
            if (FILL) band_seg[band_ptr[P.row_off + j] + at] = s;
        }
    }
}

// sign[v] = +1 inside, -1 outside.  Workgroup (row, x chunk); the row's band through LDS
__global__ __launch_bounds__(256) void polymesh_sign_kernel(const int n_poly, const PolyInfo *__restrict__ info, const double *__restrict__ seg,
                                                            const int *__restrict__ band_ptr, const int *__restrict__ band_seg,
                                                            const double h, signed char *__restrict__ sign) {
    __shared__ double lds[4 * kPolymeshChunk];
    const int row = blockIdx.x;
    const PolyInfo P = info[polymesh_poly_of_row(info, n_poly, row)];
    if ((int)blockIdx.y * 256 >= P.nx) return;                // (the same for the whole workgroup)
    const int j = row - P.row_off, ix = blockIdx.y * 256 + threadIdx.x;
    const bool active = ix < P.nx;
    const double cx = (double)(P.i0 + ix) * h, cy = (double)(P.j0 + j) * h;
    const int b0 = band_ptr[row], b1 = band_ptr[row + 1];
    bool in = false;
    for (int c0 = b0; c0 < b1; c0 += kPolymeshChunk) {
        __syncthreads();
        if (c0 + (int)threadIdx.x < b1) {
            const double *s = seg + 4 * (long long)band_seg[c0 + threadIdx.x];
            lds[4 * threadIdx.x] = s[0];
            lds[4 * threadIdx.x + 1] = s[1];
            lds[4 * threadIdx.x + 2] = s[2];
            lds[4 * threadIdx.x + 3] = s[3];
        }
        __syncthreads();
        const int n = min(kPolymeshChunk, b1 - c0);
        if (active)
            for (int k = 0; k < n; ++k) {
                const double xj = lds[4 * k], yj = lds[4 * k + 1], xi = lds[4 * k + 2], yi = lds[4 * k + 3];
                if ((yi > cy) != (yj > cy) && cx < (xj - xi) * (cy - yi) / (yj - yi) + xi) in = !in;
            }
    }
    if (active) sign[P.lat_off + j * P.nx + ix] = in ? 1 : -1;
}

// T[3 v + f] = the cut parameter of the edge of family f that starts at v, -1.0 where the ends agree or the edge leaves the lattice
__global__ __launch_bounds__(256) void polymesh_cut_kernel(const int n_poly, const PolyInfo *__restrict__ info, const double *__restrict__ seg,
                                                           const int *__restrict__ band_ptr, const int *__restrict__ band_seg,
                                                           const double h, const signed char *__restrict__ sign, double *__restrict__ T) {
    __shared__ double lds[4 * kPolymeshChunk];
    const int row = blockIdx.x;
    const PolyInfo P = info[polymesh_poly_of_row(info, n_poly, row)];
    if ((int)blockIdx.y * 256 >= P.nx) return;
    const int j = row - P.row_off, ix = blockIdx.y * 256 + threadIdx.x;
    const bool active = ix < P.nx;
    const int gv = P.lat_off + j * P.nx + ix;
    const double ax = (double)(P.i0 + ix) * h, ay = (double)(P.j0 + j) * h;
    const double bx = (double)(P.i0 + ix + 1) * h, by = (double)(P.j0 + j + 1) * h;
    const double ex = bx - ax, ny_ = by - ay;                 // E = (ex, 0), N = (0, ny_), NE = (ex, ny_)
    const bool right = active && ix + 1 < P.nx, up = active && j + 1 < P.ny;
    const int sa = active ? sign[gv] : 0;
    const bool a_plus = sa > 0;
    const bool want0 = right && sign[gv + 1] != sa, want1 = up && sign[gv + P.nx] != sa, want2 = right && up && sign[gv + P.nx + 1] != sa;
    const double none = a_plus ? INFINITY : -INFINITY;
    double best0 = none, best1 = none, best2 = none;
    const int b0 = band_ptr[row], b1 = band_ptr[row + 1];
    for (int c0 = b0; c0 < b1; c0 += kPolymeshChunk) {
        __syncthreads();
        if (c0 + (int)threadIdx.x < b1) {
            const double *s = seg + 4 * (long long)band_seg[c0 + threadIdx.x];
            lds[4 * threadIdx.x] = s[0];
            lds[4 * threadIdx.x + 1] = s[1];
            lds[4 * threadIdx.x + 2] = s[2];
            lds[4 * threadIdx.x + 3] = s[3];
        }
        __syncthreads();
        const int n = min(kPolymeshChunk, b1 - c0);
        if (want0 || want1 || want2)
            for (int k = 0; k < n; ++k) {
                const double px = lds[4 * k], py = lds[4 * k + 1];
                const double sx = lds[4 * k + 2] - px, sy = lds[4 * k + 3] - py;
                const double wx = px - ax, wy = py - ay;
                const double wxs = wx * sy - wy * sx;
                auto meet = [&](double rx, double ry, double &best) {
                    const double den = rx * sy - ry * sx;
                    const double t = wxs / den, u = (wx * ry - wy * rx) / den;
                    if (den != 0.0 && t >= 0.0 && t <= 1.0 && u >= 0.0 && u <= 1.0) best = a_plus ? fmin(best, t) : fmax(best, t);
                };
                if (want0) meet(ex, 0.0, best0);
                if (want1) meet(0.0, ny_, best1);
                if (want2) meet(ex, ny_, best2);
            }
    }
    if (active) {
        T[3 * (long long)gv] = want0 ? (isfinite(best0) ? best0 : 0.5) : -1.0;
        T[3 * (long long)gv + 1] = want1 ? (isfinite(best1) ? best1 : 0.5) : -1.0;
        T[3 * (long long)gv + 2] = want2 ? (isfinite(best2) ? best2 : 0.5) : -1.0;
    }
}

// state[v] = 0 for a snapped vertex, else its sign; pos[v] = where it lies
__global__ __launch_bounds__(256) void polymesh_snap_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info, const double h,
                                                            const double snap2, const signed char *__restrict__ sign,
                                                            const double *__restrict__ T, signed char *__restrict__ state,
                                                            double *__restrict__ pos) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    const double vx = (double)(P.i0 + ix) * h, vy = (double)(P.j0 + j) * h;
    double best = INFINITY, qx = vx, qy = vy;
    bool snapped = false;
    // E, N, NE from the vertex; W, S, SW towards it: (owner of the edge from the vertex, family)
    const int odi[6] = {0, 0, 0, -1, 0, -1}, odj[6] = {0, 0, 0, 0, -1, -1}, fam[6] = {0, 1, 2, 0, 1, 2};
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const int oi = ix + odi[d], oj = j + odj[d];
        if (oi < 0 || oj < 0) continue;
        const double t = T[3 * (long long)(P.lat_off + oj * P.nx + oi) + fam[d]];
        if (!(t >= 0.0)) continue;
        const int fdi = fam[d] != 1 ? 1 : 0, fdj = fam[d] != 0 ? 1 : 0;
        const double ax = (double)(P.i0 + oi) * h, ay = (double)(P.j0 + oj) * h;
        const double rx = (double)(P.i0 + oi + fdi) * h - ax, ry = (double)(P.j0 + oj + fdj) * h - ay;
        const double cx = ax + t * rx, cy = ay + t * ry, l2 = rx * rx + ry * ry;
        const double dx = cx - vx, dy = cy - vy;
        const double d2 = dx * dx + dy * dy;
        if (d2 < snap2 * l2 && d2 < best) {
            best = d2;
            qx = cx;
            qy = cy;
            snapped = true;
        }
    }
    state[gv] = snapped ? 0 : sign[gv];
    pos[2 * (long long)gv] = qx;
    pos[2 * (long long)gv + 1] = qy;
}

struct PolyFaces {
    int n;              // faces: 0, 1 or 2
    int slot[6];        // their corners, as slots of the polygon
};

// the pieces of triangle `which` (0 lower, 1 upper) of the cell whose v00 is (ix, j): the rule at the top of the file
__device__ __forceinline__ void polymesh_faces(const PolyInfo &P, const int ix, const int j, const int which, const double h,
                                               const signed char *__restrict__ state, const double *__restrict__ pos,
                                               const double *__restrict__ T, const double *__restrict__ seg,
                                               const int *__restrict__ band_ptr, const int *__restrict__ band_seg, PolyFaces &out) {
    const int nv = P.nx * P.ny;
    const int v00 = j * P.nx + ix, v10 = v00 + 1, v01 = v00 + P.nx, v11 = v01 + 1;
    // corners, and edge k (corner k -> corner k + 1) as the vertex that owns it and its family
    const int r0 = v00, r1 = which ? v11 : v10, r2 = which ? v01 : v11;
    const int o0 = v00, o1 = which ? v01 : v10, o2 = v00;
    const int f0 = which ? 2 : 0, f1 = which ? 0 : 1, f2 = which ? 1 : 2;
    const signed char *st = state + P.lat_off;
    const int s0 = st[r0], s1 = st[r1], s2 = st[r2];
    const int n_plus = (s0 > 0) + (s1 > 0) + (s2 > 0), n_minus = (s0 < 0) + (s1 < 0) + (s2 < 0);
    out.n = 0;
    const double *ps = pos + 2 * (long long)P.lat_off;
    if (n_plus == 0) {
        if (n_minus != 0) return;
        const double gx = ((ps[2 * r0] + ps[2 * r1]) + ps[2 * r2]) / 3, gy = ((ps[2 * r0 + 1] + ps[2 * r1 + 1]) + ps[2 * r2 + 1]) / 3;
        const int row = P.row_off + j;
        if (!polymesh_inside(seg, band_seg + band_ptr[row], band_ptr[row + 1] - band_ptr[row], gx, gy)) return;
    }
    if (n_minus == 0) {
        out.n = 1;
        out.slot[0] = r0;
        out.slot[1] = r1;
        out.slot[2] = r2;
        return;
    }
    // mixed: + first, or with two + the - last
    const int first_plus = s0 > 0 ? 0 : s1 > 0 ? 1 : 2, first_minus = s0 < 0 ? 0 : s1 < 0 ? 1 : 2;
    const int rot = n_plus == 2 ? (first_minus + 1) % 3 : first_plus;
    auto pick = [rot](int k, int a0, int a1, int a2) {
        const int m = (rot + k) % 3;
        return m == 0 ? a0 : m == 1 ? a1 : a2;
    };
    const int p = pick(0, r0, r1, r2), q = pick(1, r0, r1, r2), r = pick(2, r0, r1, r2);
    const int sq = pick(1, s0, s1, s2);
    const int opq = pick(0, o0, o1, o2), oqr = pick(1, o0, o1, o2), orp = pick(2, o0, o1, o2);
    const int fpq = pick(0, f0, f1, f2), fqr = pick(1, f0, f1, f2), frp = pick(2, f0, f1, f2);
    const int cpq = nv + 3 * opq + fpq, cqr = nv + 3 * oqr + fqr, crp = nv + 3 * orp + frp;
    auto put = [&out](int a, int b, int c) {
        out.slot[3 * out.n] = a;
        out.slot[3 * out.n + 1] = b;
        out.slot[3 * out.n + 2] = c;
        ++out.n;
    };
    if (n_plus == 1 && n_minus == 2) {
        put(p, cpq, crp);
    } else if (n_plus == 1) {
        if (sq == 0) put(p, q, crp); else put(p, cpq, r);
    } else {
        // the quadrilateral p, q, cut qr, cut rp along its shorter diagonal
        auto cut_at = [&](int owner, int f, double &cx, double &cy) {
            const int oi = owner % P.nx, oj = owner / P.nx;
            const int fdi = f != 1 ? 1 : 0, fdj = f != 0 ? 1 : 0;
            const double t = T[3 * (long long)(P.lat_off + owner) + f];
            const double ax = (double)(P.i0 + oi) * h, ay = (double)(P.j0 + oj) * h;
            const double rx = (double)(P.i0 + oi + fdi) * h - ax, ry = (double)(P.j0 + oj + fdj) * h - ay;
            cx = ax + t * rx;
            cy = ay + t * ry;
        };
        double qrx, qry, rpx, rpy;
        cut_at(oqr, fqr, qrx, qry);
        cut_at(orp, frp, rpx, rpy);
        const double ex = qrx - ps[2 * p], ey = qry - ps[2 * p + 1];
        const double fx = rpx - ps[2 * q], fy = rpy - ps[2 * q + 1];
        const double d1 = ex * ex + ey * ey, d2 = fx * fx + fy * fy;
        if (d1 <= d2) {
            put(p, q, cqr);
            put(p, cqr, crp);
        } else {
            put(p, q, crp);
            put(q, cqr, crp);
        }
    }
}

constexpr int kPolymeshMaxLevels = 6;

struct PolyLevels {
    int n;                              // levels, 1 .. kPolymeshMaxLevels
    int t[kPolymeshMaxLevels];          // t[0] = 0
};

// plain[v] = 1 when v is the v00 of a cell whose four corners are +
__global__ __launch_bounds__(256) void polymesh_plain_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info,
                                                             const signed char *__restrict__ state, unsigned char *__restrict__ plain) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    bool is = false;
    if (ix + 1 < P.nx && j + 1 < P.ny) is = state[gv] > 0 && state[gv + 1] > 0 && state[gv + P.nx] > 0 && state[gv + P.nx + 1] > 0;
    plain[gv] = is ? 1 : 0;
}

// thread = (polygon, seed): the seed's cell, when the polygon's lattice has it, is not plain (idempotent plain stores)
__global__ __launch_bounds__(256) void polymesh_seed_kernel(const int n_seed, const int n_poly, const PolyInfo *__restrict__ info,
                                                            const double *__restrict__ seed, const double h, unsigned char *plain) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_seed * n_poly) return;
    const PolyInfo P = info[i / n_seed];
    const int k = (int)(i % n_seed);
    const double fi = floor(seed[2 * k] / h) - (double)P.i0, fj = floor(seed[2 * k + 1] / h) - (double)P.j0;
    if (fi >= 0.0 && fi < (double)(P.nx - 1) && fj >= 0.0 && fj < (double)(P.ny - 1)) plain[P.lat_off + (int)fj * P.nx + (int)fi] = 0;
}

// drow[v] = the least k <= cap with cell ci - k or ci + k of the row not plain (outside the row: not plain), else cap
__global__ __launch_bounds__(256) void polymesh_rowdist_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info,
                                                               const unsigned char *__restrict__ plain, const int cap, int *__restrict__ drow) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    int k = 0;
    if (ix + 1 < P.nx && j + 1 < P.ny) {
        const unsigned char *row = plain + (gv - ix);
        for (; k < cap; ++k) {
            if (ix - k < 0 || ix + k >= P.nx - 1) break;
            if (!row[ix - k] || !row[ix + k]) break;
        }
    }
    drow[gv] = k;
}

// d[v] = min over k of max(k, drow of the rows cj - k and cj + k) (outside the lattice: 0), capped as drow is.  Adjacent
// threads read adjacent cells of every row they visit
__global__ __launch_bounds__(256) void polymesh_coldist_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info,
                                                               const int *__restrict__ drow, int *__restrict__ d) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    int best = 0;
    if (ix + 1 < P.nx && j + 1 < P.ny) {
        best = drow[gv];
        for (int k = 1; k < best; ++k) {
            const int below = j - k >= 0 ? drow[gv - k * P.nx] : 0, above = j + k < P.ny - 1 ? drow[gv + k * P.nx] : 0;
            best = min(best, max(k, min(below, above)));
        }
    }
    d[gv] = best;
}

// level l >= 1: bmin[a] at the anchor a of every aligned block of 2^l x 2^l cells inside the lattice = the least d of the
// block, from the four blocks of level l - 1 (bmin of level 0 is d; in place: a block's anchor is read by that block alone);
// bit l of ok[a] set when it is at least t[l]
__global__ __launch_bounds__(256) void polymesh_blockmin_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info,
                                                                const int l, const int t_l, int *bmin, unsigned char *ok) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    const int s = 1 << l, hs = s >> 1;
    if (((P.i0 + ix) & (s - 1)) != 0 || ((P.j0 + j) & (s - 1)) != 0 || ix + s > P.nx - 1 || j + s > P.ny - 1) return;
    const int m = min(min(bmin[gv], bmin[gv + hs]), min(bmin[gv + hs * P.nx], bmin[gv + hs * P.nx + hs]));
    bmin[gv] = m;
    if (m >= t_l) ok[gv] = (unsigned char)(ok[gv] | (1u << l));
}

// level[v] of the cell whose v00 is v (0 where there is none); cells[p * kPolymeshMaxLevels + l] += the cells of level l
__global__ __launch_bounds__(256) void polymesh_level_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info,
                                                             const int n_level, const unsigned char *__restrict__ ok,
                                                             signed char *__restrict__ level, int *cells) {
    __shared__ int hist[kPolymeshMaxLevels];
    __shared__ int first_poly, mixed;
    const int gv = blockIdx.x * 256 + threadIdx.x;
    const bool live = gv < n_lat;
    const int p = polymesh_poly_of_vertex(info, n_poly, live ? gv : n_lat - 1);
    if (threadIdx.x < kPolymeshMaxLevels) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        first_poly = p;
        mixed = 0;
    }
    __syncthreads();
    if (p != first_poly) mixed = 1;
    __syncthreads();
    const PolyInfo P = info[p];
    const int lv = (live ? gv : n_lat - 1) - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    const bool cell = live && ix + 1 < P.nx && j + 1 < P.ny;
    int lev = 0;
    if (cell)
        for (int l = n_level - 1; l >= 1; --l) {
            const int s = 1 << l, ai = ix - ((P.i0 + ix) & (s - 1)), aj = j - ((P.j0 + j) & (s - 1));
            if (ai < 0 || aj < 0 || ai + s > P.nx - 1 || aj + s > P.ny - 1) continue;
            if ((ok[P.lat_off + aj * P.nx + ai] >> l) & 1) {
                lev = l;
                break;
            }
        }
    if (live) level[gv] = (signed char)lev;
    if (cell) {
        if (mixed) atomicAdd(cells + (long long)p * kPolymeshMaxLevels + lev, 1); else atomicAdd(hist + lev, 1);
    }
    __syncthreads();
    if (!mixed && threadIdx.x < n_level && hist[threadIdx.x] > 0)
        atomicAdd(cells + (long long)first_poly * kPolymeshMaxLevels + threadIdx.x, hist[threadIdx.x]);
}

// the faces of the leaf of level l >= 1 whose anchor cell's v00 is (ix, j), handed one by one to put(a, b, c) as slots:
// the rule at the top of the file.  level: the polygon's own (level + lat_off)
template <typename Put>
__device__ __forceinline__ void polymesh_leaf(const PolyInfo &P, const int ix, const int j, const int l,
                                              const signed char *__restrict__ level, Put put) {
    const int s = 1 << l, hs = s >> 1, nx = P.nx;
    auto level_at = [&](int ci, int cj) {
        return ci < 0 || cj < 0 || ci >= nx - 1 || cj >= P.ny - 1 ? 0 : (int)level[cj * nx + ci];
    };
    const bool hang_s = level_at(ix, j - 1) < l, hang_e = level_at(ix + s, j) < l, hang_n = level_at(ix, j + s) < l,
               hang_w = level_at(ix - 1, j) < l;
    const int v00 = j * nx + ix, v10 = v00 + s, v01 = v00 + s * nx, v11 = v01 + s;
    if (!(hang_s || hang_e || hang_n || hang_w)) {
        put(v00, v10, v11);
        put(v00, v11, v01);
        return;
    }
    const int c = v00 + hs * nx + hs;
    int prev = v00;
    auto step = [&](int v) {
        put(c, prev, v);
        prev = v;
    };
    if (hang_s) step(v00 + hs);
    step(v10);
    if (hang_e) step(v10 + hs * nx);
    step(v11);
    if (hang_n) step(v01 + hs);
    step(v01);
    if (hang_w) step(v00 + hs * nx);
    step(v00);
}

__device__ __forceinline__ bool polymesh_is_anchor(const PolyInfo &P, const int ix, const int j, const int l) {
    const int s = 1 << l;
    return ((P.i0 + ix) & (s - 1)) == 0 && ((P.j0 + j) & (s - 1)) == 0;
}

// fcount[2 v + which] = the faces of the two triangles of the cell whose v00 is v; flag = 1 on every slot they name.
// GRADED: a cell of a leaf of level >= 1 counts the leaf's faces as its lower triangle's when it is the anchor, else none
template <bool GRADED>
__global__ __launch_bounds__(256) void polymesh_count_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info, const double h,
                                                             const signed char *__restrict__ state, const double *__restrict__ pos,
                                                             const double *__restrict__ T, const double *__restrict__ seg,
                                                             const int *__restrict__ band_ptr, const int *__restrict__ band_seg,
                                                             const signed char *__restrict__ level, int *__restrict__ fcount, int *flag) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    if (GRADED) {
        const int l = level[gv];
        if (l > 0) {
            int n = 0;
            int *fl = flag + 4 * (long long)P.lat_off;
            if (polymesh_is_anchor(P, ix, j, l))
                polymesh_leaf(P, ix, j, l, level + P.lat_off, [&](int a, int b, int c) {
                    fl[a] = 1;
                    fl[b] = 1;
                    fl[c] = 1;
                    ++n;
                });
            fcount[2 * (long long)gv] = n;
            fcount[2 * (long long)gv + 1] = 0;
            return;
        }
    }
    for (int which = 0; which < 2; ++which) {
        PolyFaces f;
        f.n = 0;
        if (ix + 1 < P.nx && j + 1 < P.ny) polymesh_faces(P, ix, j, which, h, state, pos, T, seg, band_ptr, band_seg, f);
        fcount[2 * (long long)gv + which] = f.n;
        for (int k = 0; k < 3 * f.n; ++k) flag[4 * (long long)P.lat_off + f.slot[k]] = 1;      // (idempotent plain stores)
    }
}

// vbase[p] = the vertices in front of polygon p, fbase[p] = the faces, p = 0 .. n_poly
__global__ __launch_bounds__(256) void polymesh_base_kernel(const int n_poly, const PolyInfo *__restrict__ info, const int *__restrict__ vnum,
                                                            const int *__restrict__ foff, int *__restrict__ vbase, int *__restrict__ fbase) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n_poly) return;
    vbase[p] = vnum[4 * (long long)info[p].lat_off];
    fbase[p] = foff[2 * (long long)info[p].lat_off];
}

// thread i = a slot of the batch (4 per lattice vertex): a flagged one writes its vertex
__global__ __launch_bounds__(256) void polymesh_vertex_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info, const double h,
                                                              const signed char *__restrict__ state, const double *__restrict__ pos,
                                                              const double *__restrict__ T, const int *__restrict__ flag,
                                                              const int *__restrict__ vnum, double *__restrict__ xy, int *__restrict__ kind) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * (long long)n_lat || !flag[i]) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, (int)(i >> 2))];
    const int nv = P.nx * P.ny, slot = (int)(i - 4 * (long long)P.lat_off);
    const long long g = vnum[i];
    if (slot < nv) {
        const long long gv = P.lat_off + slot;
        xy[2 * g] = pos[2 * gv];
        xy[2 * g + 1] = pos[2 * gv + 1];
        kind[g] = state[gv] == 0 ? 1 : 0;
        return;
    }
    const int owner = (slot - nv) / 3, f = (slot - nv) % 3;
    const int oi = owner % P.nx, oj = owner / P.nx;
    const int fdi = f != 1 ? 1 : 0, fdj = f != 0 ? 1 : 0;
    const double t = T[3 * (long long)(P.lat_off + owner) + f];
    const double ax = (double)(P.i0 + oi) * h, ay = (double)(P.j0 + oj) * h;
    const double rx = (double)(P.i0 + oi + fdi) * h - ax, ry = (double)(P.j0 + oj + fdj) * h - ay;
    xy[2 * g] = ax + t * rx;
    xy[2 * g + 1] = ay + t * ry;
    kind[g] = 2;
}

// the faces of every cell at their offsets, with the vertex numbers of their polygon
template <bool GRADED>
__global__ __launch_bounds__(256) void polymesh_face_kernel(const int n_lat, const int n_poly, const PolyInfo *__restrict__ info, const double h,
                                                            const signed char *__restrict__ state, const double *__restrict__ pos,
                                                            const double *__restrict__ T, const double *__restrict__ seg,
                                                            const int *__restrict__ band_ptr, const int *__restrict__ band_seg,
                                                            const signed char *__restrict__ level, const int *__restrict__ vnum,
                                                            const int *__restrict__ foff, int *__restrict__ tri) {
    const int gv = blockIdx.x * 256 + threadIdx.x;
    if (gv >= n_lat) return;
    const PolyInfo P = info[polymesh_poly_of_vertex(info, n_poly, gv)];
    const int lv = gv - P.lat_off, ix = lv % P.nx, j = lv / P.nx;
    if (ix + 1 >= P.nx || j + 1 >= P.ny) return;
    const int *num = vnum + 4 * (long long)P.lat_off;
    const int base = num[0];
    if (GRADED) {
        const int l = level[gv];
        if (l > 0) {
            if (!polymesh_is_anchor(P, ix, j, l)) return;
            int *out = tri + 3 * (long long)foff[2 * (long long)gv];
            polymesh_leaf(P, ix, j, l, level + P.lat_off, [&](int a, int b, int c) {
                out[0] = num[a] - base;
                out[1] = num[b] - base;
                out[2] = num[c] - base;
                out += 3;
            });
            return;
        }
    }
    for (int which = 0; which < 2; ++which) {
        PolyFaces f;
        polymesh_faces(P, ix, j, which, h, state, pos, T, seg, band_ptr, band_seg, f);
        int *out = tri + 3 * (long long)foff[2 * (long long)gv + which];
        for (int k = 0; k < 3 * f.n; ++k) out[k] = num[f.slot[k]] - base;
    }
}

}  // namespace padne

using namespace padne;

struct padne_polymesh {
    padne_ctx *owner = nullptr;
    int64_t n_poly = 0, n_vert = 0, n_tri = 0;
    // device (the owner's pool)
    double *xy = nullptr;
    int *tri = nullptr, *kind = nullptr;
};

static void polymesh_free(padne_polymesh *pm) {
    if (pm == nullptr) return;
    void *blocks[] = {pm->xy, pm->tri, pm->kind};
    for (void *p : blocks)
        if (p) pool_free(pm->owner, p);
    delete pm;
}

template <typename T> static int polymesh_alloc(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

// both entries: lv.n == 1 is the uniform mesh, and runs what it ran before there were levels
static int polymesh_create(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr, const double *ring_xy,
                           double h, double snap, const PolyLevels &lv, int64_t n_seed, const double *seed_xy,
                           int64_t *vertex_count_out, int64_t *face_count_out, int64_t *level_cells_out, padne_polymesh **out) {
    PADNE_REQUIRE(poly_ring_ptr && ring_ptr && ring_xy && vertex_count_out && face_count_out, "null argument");
    PADNE_REQUIRE(n_poly >= 1 && n_poly < (1LL << 24), "a batch holds at least one polygon");
    PADNE_REQUIRE(h > 0.0 && std::isfinite(h), "the spacing must be positive");
    PADNE_REQUIRE(snap > 0.0 && snap < 0.5, "snap must lie in (0, 1/2)");
    PADNE_REQUIRE(poly_ring_ptr[0] == 0 && ring_ptr[0] == 0, "offset tables must start at 0");
    // ---- the lattices and the segments, on the host: one pass over the rings
    std::vector<PolyInfo> info((size_t)n_poly + 1);
    std::vector<double> seg;
    std::vector<int> seg_poly;
    long long n_lat = 0, n_row = 0, max_nx = 0;
    double band_bound = 0.0;
    for (int64_t p = 0; p < n_poly; ++p) {
        PADNE_REQUIRE(poly_ring_ptr[p + 1] > poly_ring_ptr[p], "a polygon has at least its exterior ring");
        double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        for (int64_t r = poly_ring_ptr[p]; r < poly_ring_ptr[p + 1]; ++r) {
            const int64_t v0 = ring_ptr[r], n = ring_ptr[r + 1] - v0;
            PADNE_REQUIRE(n >= 3, "a ring has at least 3 vertices");
            PADNE_REQUIRE((long long)seg_poly.size() + n < 0x7fffffffLL, "too many segments for 32-bit indices");
            for (int64_t k = 0; k < n; ++k) {
                const int64_t prev = v0 + (k + n - 1) % n, cur = v0 + k;
                const double xj = ring_xy[2 * prev], yj = ring_xy[2 * prev + 1], xi = ring_xy[2 * cur], yi = ring_xy[2 * cur + 1];
                PADNE_REQUIRE(std::isfinite(xi) && std::isfinite(yi), "a coordinate is not finite");
                seg.insert(seg.end(), {xj, yj, xi, yi});
                seg_poly.push_back((int)p);
                xmin = std::fmin(xmin, xi);
                xmax = std::fmax(xmax, xi);
                ymin = std::fmin(ymin, yi);
                ymax = std::fmax(ymax, yi);
                band_bound += std::fabs(yi - yj) / h + 5.0;
            }
        }
        const double fi0 = std::floor(xmin / h) - 1.0, fj0 = std::floor(ymin / h) - 1.0;
        const double fnx = std::ceil(xmax / h) + 1.0 - fi0 + 1.0, fny = std::ceil(ymax / h) + 1.0 - fj0 + 1.0;
        PADNE_REQUIRE(std::fabs(fi0) < 1e9 && std::fabs(fj0) < 1e9 && std::fabs(fi0 + fnx) < 1e9 && std::fabs(fj0 + fny) < 1e9,
                      "lattice indices beyond 32 bits: the spacing is too small for these coordinates");
        PADNE_REQUIRE(fnx * fny <= (double)kPolymeshMaxLattice, "a lattice of more than 2^24 vertices: raise the spacing");
        PolyInfo &P = info[(size_t)p];
        P.lat_off = (int)n_lat;
        P.row_off = (int)n_row;
        P.i0 = (int)fi0;
        P.j0 = (int)fj0;
        P.nx = (int)fnx;
        P.ny = (int)fny;
        n_lat += (long long)P.nx * P.ny;
        n_row += P.ny;
        max_nx = P.nx > max_nx ? P.nx : max_nx;
        PADNE_REQUIRE(n_lat <= kPolymeshMaxBatch, "a batch of more than 2^27 lattice vertices: split it");
    }
    PADNE_REQUIRE(band_bound < 2147483647.0, "the band index would overflow 32-bit indices: raise the spacing");
    info[(size_t)n_poly] = PolyInfo{(int)n_lat, (int)n_row, 0, 0, 0, 0};
    const int n_seg = (int)seg_poly.size(), np = (int)n_poly, nl = (int)n_lat, nr = (int)n_row;

    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_polymesh *pm = new padne_polymesh;
    pm->owner = ctx;
    pm->n_poly = n_poly;
    struct Guard {      // an error path hands everything back
        padne_polymesh *pm;
        ~Guard() { polymesh_free(pm); }
    } guard{pm};
    Scratch sc(ctx);
    PolyInfo *d_info = nullptr;
    double *d_seg = nullptr, *d_T = nullptr, *d_pos = nullptr;
    int *d_seg_poly = nullptr, *d_count = nullptr, *d_band_ptr = nullptr, *d_band_seg = nullptr, *d_fcount = nullptr, *d_foff = nullptr,
        *d_flag = nullptr, *d_vnum = nullptr, *d_vbase = nullptr, *d_fbase = nullptr;
    signed char *d_sign = nullptr, *d_state = nullptr, *d_level = nullptr;
    const bool graded = lv.n > 1;
    PADNE_TRY(sc.alloc(&d_info, (size_t)n_poly + 1));
    PADNE_TRY(sc.alloc(&d_seg, 4 * (size_t)n_seg));
    PADNE_TRY(sc.alloc(&d_seg_poly, (size_t)n_seg));
    PADNE_TRY(sc.alloc(&d_count, (size_t)nr));
    PADNE_TRY(sc.alloc(&d_band_ptr, (size_t)nr + 1));
    PADNE_TRY(sc.alloc(&d_sign, (size_t)nl));
    PADNE_TRY(sc.alloc(&d_state, (size_t)nl));
    PADNE_TRY(sc.alloc(&d_T, 3 * (size_t)nl));
    PADNE_TRY(sc.alloc(&d_pos, 2 * (size_t)nl));
    PADNE_TRY(sc.alloc(&d_fcount, 2 * (size_t)nl));
    PADNE_TRY(sc.alloc(&d_foff, 2 * (size_t)nl + 1));
    PADNE_TRY(sc.alloc(&d_flag, 4 * (size_t)nl));
    PADNE_TRY(sc.alloc(&d_vnum, 4 * (size_t)nl + 1));
    PADNE_TRY(sc.alloc(&d_vbase, (size_t)n_poly + 1));
    PADNE_TRY(sc.alloc(&d_fbase, (size_t)n_poly + 1));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_info, info.data(), sizeof(PolyInfo) * ((size_t)n_poly + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_seg, seg.data(), sizeof(double) * 4 * (size_t)n_seg, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_seg_poly, seg_poly.data(), sizeof(int) * (size_t)n_seg, hipMemcpyHostToDevice, s));

    // ---- the band index: count, scan, fill
    int64_t n_band = 0, n_vert = 0, n_tri = 0;
    PADNE_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)nr, s));
    hipLaunchKernelGGL(polymesh_band_kernel<false>, dim3(nblk(n_seg)), dim3(256), 0, s, n_seg, (const double *)d_seg, (const int *)d_seg_poly,
                       (const PolyInfo *)d_info, h, d_count, (const int *)nullptr, (int *)nullptr);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_TRY(exclusive_scan_i32(ctx, d_count, d_band_ptr, nr, &n_band));
    PADNE_TRY(sc.alloc(&d_band_seg, (size_t)n_band));
    PADNE_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)nr, s));
    hipLaunchKernelGGL(polymesh_band_kernel<true>, dim3(nblk(n_seg)), dim3(256), 0, s, n_seg, (const double *)d_seg, (const int *)d_seg_poly,
                       (const PolyInfo *)d_info, h, d_count, (const int *)d_band_ptr, d_band_seg);
    PADNE_HIP_CHECK(hipGetLastError());

    // ---- sign, cuts, snap
    const dim3 rows_grid((unsigned)nr, (unsigned)((max_nx + 255) / 256));
    hipLaunchKernelGGL(polymesh_sign_kernel, rows_grid, dim3(256), 0, s, np, (const PolyInfo *)d_info, (const double *)d_seg,
                       (const int *)d_band_ptr, (const int *)d_band_seg, h, d_sign);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(polymesh_cut_kernel, rows_grid, dim3(256), 0, s, np, (const PolyInfo *)d_info, (const double *)d_seg,
                       (const int *)d_band_ptr, (const int *)d_band_seg, h, (const signed char *)d_sign, d_T);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(polymesh_snap_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h, snap * snap,
                       (const signed char *)d_sign, (const double *)d_T, d_state, d_pos);
    PADNE_HIP_CHECK(hipGetLastError());

    // ---- graded: plain cells, seeds, the capped distance, the block minima level by level, the level of every cell
    std::vector<int> cells;
    if (graded) {
        unsigned char *d_plain = nullptr, *d_ok = nullptr;
        int *d_drow = nullptr, *d_dist = nullptr, *d_cells = nullptr;
        double *d_seed = nullptr;
        PADNE_TRY(sc.alloc(&d_plain, (size_t)nl));
        PADNE_TRY(sc.alloc(&d_ok, (size_t)nl));
        PADNE_TRY(sc.alloc(&d_drow, (size_t)nl));
        PADNE_TRY(sc.alloc(&d_dist, (size_t)nl));
        PADNE_TRY(sc.alloc(&d_level, (size_t)nl));
        PADNE_TRY(sc.alloc(&d_cells, (size_t)n_poly * kPolymeshMaxLevels));
        hipLaunchKernelGGL(polymesh_plain_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info,
                           (const signed char *)d_state, d_plain);
        PADNE_HIP_CHECK(hipGetLastError());
        if (n_seed > 0) {
            PADNE_TRY(sc.alloc(&d_seed, 2 * (size_t)n_seed));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_seed, seed_xy, sizeof(double) * 2 * (size_t)n_seed, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(polymesh_seed_kernel, dim3(nblk((long long)n_seed * n_poly)), dim3(256), 0, s, (int)n_seed, np,
                               (const PolyInfo *)d_info, (const double *)d_seed, h, d_plain);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(polymesh_rowdist_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info,
                           (const unsigned char *)d_plain, lv.t[lv.n - 1], d_drow);
        PADNE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(polymesh_coldist_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, (const int *)d_drow,
                           d_dist);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemsetAsync(d_ok, 0, (size_t)nl, s));
        PADNE_HIP_CHECK(hipMemsetAsync(d_cells, 0, sizeof(int) * (size_t)n_poly * kPolymeshMaxLevels, s));
        for (int l = 1; l < lv.n; ++l) {
            hipLaunchKernelGGL(polymesh_blockmin_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, l, lv.t[l], d_dist,
                               d_ok);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(polymesh_level_kernel, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, lv.n,
                           (const unsigned char *)d_ok, d_level, d_cells);
        PADNE_HIP_CHECK(hipGetLastError());
        cells.resize((size_t)n_poly * kPolymeshMaxLevels);
        PADNE_HIP_CHECK(hipMemcpyAsync(cells.data(), d_cells, sizeof(int) * cells.size(), hipMemcpyDeviceToHost, s));
    }

    // ---- counts and flags, the two scans
    PADNE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int) * 4 * (size_t)nl, s));
    if (graded)
        hipLaunchKernelGGL(polymesh_count_kernel<true>, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h,
                           (const signed char *)d_state, (const double *)d_pos, (const double *)d_T, (const double *)d_seg,
                           (const int *)d_band_ptr, (const int *)d_band_seg, (const signed char *)d_level, d_fcount, d_flag);
    else
        hipLaunchKernelGGL(polymesh_count_kernel<false>, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h,
                           (const signed char *)d_state, (const double *)d_pos, (const double *)d_T, (const double *)d_seg,
                           (const int *)d_band_ptr, (const int *)d_band_seg, (const signed char *)nullptr, d_fcount, d_flag);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_TRY(exclusive_scan_i32(ctx, d_flag, d_vnum, 4 * (int64_t)nl, &n_vert));
    PADNE_TRY(exclusive_scan_i32(ctx, d_fcount, d_foff, 2 * (int64_t)nl, &n_tri));
    hipLaunchKernelGGL(polymesh_base_kernel, dim3(nblk(n_poly + 1)), dim3(256), 0, s, np, (const PolyInfo *)d_info, (const int *)d_vnum,
                       (const int *)d_foff, d_vbase, d_fbase);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<int> vbase((size_t)n_poly + 1), fbase((size_t)n_poly + 1);
    PADNE_HIP_CHECK(hipMemcpyAsync(vbase.data(), d_vbase, sizeof(int) * ((size_t)n_poly + 1), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(fbase.data(), d_fbase, sizeof(int) * ((size_t)n_poly + 1), hipMemcpyDeviceToHost, s));

    // ---- emit
    pm->n_vert = n_vert;
    pm->n_tri = n_tri;
    PADNE_TRY(polymesh_alloc(ctx, &pm->xy, 2 * (size_t)n_vert));
    PADNE_TRY(polymesh_alloc(ctx, &pm->kind, (size_t)n_vert));
    PADNE_TRY(polymesh_alloc(ctx, &pm->tri, 3 * (size_t)n_tri));
    hipLaunchKernelGGL(polymesh_vertex_kernel, dim3(nblk(4 * (long long)nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h,
                       (const signed char *)d_state, (const double *)d_pos, (const double *)d_T, (const int *)d_flag, (const int *)d_vnum,
                       pm->xy, pm->kind);
    PADNE_HIP_CHECK(hipGetLastError());
    if (graded)
        hipLaunchKernelGGL(polymesh_face_kernel<true>, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h,
                           (const signed char *)d_state, (const double *)d_pos, (const double *)d_T, (const double *)d_seg,
                           (const int *)d_band_ptr, (const int *)d_band_seg, (const signed char *)d_level, (const int *)d_vnum,
                           (const int *)d_foff, pm->tri);
    else
        hipLaunchKernelGGL(polymesh_face_kernel<false>, dim3(nblk(nl)), dim3(256), 0, s, nl, np, (const PolyInfo *)d_info, h,
                           (const signed char *)d_state, (const double *)d_pos, (const double *)d_T, (const double *)d_seg,
                           (const int *)d_band_ptr, (const int *)d_band_seg, (const signed char *)nullptr, (const int *)d_vnum,
                           (const int *)d_foff, pm->tri);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t p = 0; p < n_poly; ++p) {
        vertex_count_out[p] = vbase[(size_t)p + 1] - vbase[(size_t)p];
        face_count_out[p] = fbase[(size_t)p + 1] - fbase[(size_t)p];
        if (level_cells_out == nullptr) continue;
        const PolyInfo &P = info[(size_t)p];
        for (int l = 0; l < lv.n; ++l)
            level_cells_out[p * lv.n + l] = graded ? cells[(size_t)p * kPolymeshMaxLevels + l] : (int64_t)(P.nx - 1) * (P.ny - 1);
    }
    guard.pm = nullptr;
    *out = pm;
    return PADNE_OK;
}

extern "C" int padne_polymesh_create(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                                     const double *ring_xy, double h, double snap, int64_t *vertex_count_out,
                                     int64_t *face_count_out, padne_polymesh **out) {
    PADNE_REQUIRE(ctx && out, "null argument");
    *out = nullptr;
    return polymesh_create(ctx, n_poly, poly_ring_ptr, ring_ptr, ring_xy, h, snap, PolyLevels{1, {0}}, 0, nullptr, vertex_count_out,
                           face_count_out, nullptr, out);
}

extern "C" int padne_polymesh_create_graded(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                                            const double *ring_xy, double h, double snap, int64_t n_level,
                                            const int32_t *threshold, int64_t n_seed, const double *seed_xy,
                                            int64_t *vertex_count_out, int64_t *face_count_out, int64_t *level_cells_out,
                                            padne_polymesh **out) {
    PADNE_REQUIRE(ctx && out, "null argument");
    *out = nullptr;
    PADNE_REQUIRE(n_level >= 1 && n_level <= kPolymeshMaxLevels, "1 to 6 levels");
    PADNE_REQUIRE(threshold != nullptr, "null argument");
    PADNE_REQUIRE(threshold[0] == 0, "the threshold of level 0 is 0");
    PolyLevels lv{(int)n_level, {0}};
    for (int l = 1; l < lv.n; ++l) {
        PADNE_REQUIRE((long long)threshold[l] >= (long long)threshold[l - 1] + (1LL << (l - 1)),
                      "a threshold must be at least the one below it plus 2^(l - 1): the quadtree would not be balanced");
        lv.t[l] = threshold[l];
    }
    PADNE_REQUIRE(n_seed >= 0 && n_seed < (1LL << 24), "the number of seeds");
    PADNE_REQUIRE(n_seed == 0 || seed_xy != nullptr, "null argument");
    for (int64_t k = 0; k < 2 * n_seed; ++k) PADNE_REQUIRE(std::isfinite(seed_xy[k]), "a seed coordinate is not finite");
    PADNE_REQUIRE(n_poly < 1 || n_seed * n_poly < 0x7fffffffLL, "too many (seed, polygon) pairs for 32-bit indices");
    return polymesh_create(ctx, n_poly, poly_ring_ptr, ring_ptr, ring_xy, h, snap, lv, n_seed, seed_xy, vertex_count_out,
                           face_count_out, level_cells_out, out);
}

extern "C" int padne_polymesh_fetch(padne_ctx *ctx, const padne_polymesh *pm, double *xy_out, int32_t *tri_out, int32_t *kind_out) {
    PADNE_REQUIRE(ctx && pm, "null argument");
    PADNE_REQUIRE(ctx == pm->owner, "a batch of meshes is fetched through the context that made it");
    PADNE_REQUIRE(pm->n_vert == 0 || (xy_out && kind_out), "null argument");
    PADNE_REQUIRE(pm->n_tri == 0 || tri_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (pm->n_vert > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(xy_out, pm->xy, sizeof(double) * 2 * (size_t)pm->n_vert, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(kind_out, pm->kind, sizeof(int32_t) * (size_t)pm->n_vert, hipMemcpyDeviceToHost, s));
    }
    if (pm->n_tri > 0) PADNE_HIP_CHECK(hipMemcpyAsync(tri_out, pm->tri, sizeof(int32_t) * 3 * (size_t)pm->n_tri, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_polymesh_arrays(const padne_polymesh *pm, const void **xy_dev, const void **tri_dev, const void **kind_dev) {
    PADNE_REQUIRE(pm && xy_dev && tri_dev && kind_dev, "null argument");
    *xy_dev = pm->xy;
    *tri_dev = pm->tri;
    *kind_dev = pm->kind;
    return PADNE_OK;
}

extern "C" int padne_polymesh_destroy(padne_polymesh *pm) {
    if (pm == nullptr) return PADNE_OK;
    if (pm->owner) {
        (void)hipSetDevice(pm->owner->device);
        (void)hipStreamSynchronize(pm->owner->stream);
    }
    polymesh_free(pm);
    return PADNE_OK;
}
