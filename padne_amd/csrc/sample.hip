// Field sampler: the solved fields read out at points, along lines and on rasters ("Sampling").
//
//   padne_sampler_create : meshes + potentials -> device-resident sampler with a point-location index per layer
//   padne_sampler_points : uploaded query points   -> owner face, V, J, p per point
//   padne_sampler_raster : pixel centres formed by the kernel -> the same four as images
//   padne_sampler_set_fields / _field_points / _field_raster : a block of temperature fields on the same handle, every
//                          field read out at the one owner of a query ("Thermal images")
//
// The owner rule (what "the face that contains q" means, bit for bit):
//   edge (i, k) of a face is evaluated from its lower global vertex to its higher one, side = orient(P, Q, q), and negated
//   where the face runs the edge the other way, so the two faces of an edge see the same number with opposite signs.  A
//   face contains q when its three sides are all >= 0 or all <= 0 and not all zero; the owner is the containing face with
//   the lowest global index.  The index only proposes candidates; tests/sampling_ref.py states the rule by brute force.
//
// This file is compiled with -ffp-contract=off, like assemble.hip: every expression rounds as written.
#include "error.hpp"
#include "locate.hpp"

#include <float.h>

#include <algorithm>
#include <chrono>
#include <cmath>

namespace padne {

constexpr long long kMaxSamples = 1LL << 26;      // query points / pixels of one call

struct RasterSpec {
    double x0, y0, dx, dy;
    long long width;
};

// The bins face f may own a point of: those its bounding box meets, grown by a margin that covers the points the rounding
// of orient() can add to it.  With S the longer side of the box, A the area and d the distance of q from the face, one of
// the three exact sides is <= -d A / L_max and another >= d A / (2 L_max) (they sum to 2 A), while a computed side is off
// by at most 8 eps S (S + d): beyond d = 64 eps S^3 / A the signs are the exact ones and the face does not contain q
// (for 16 sqrt(2) eps S^2 / A <= 1/8).  A face too thin for that bound may own points anywhere: it is listed in every bin.
__device__ __forceinline__ bool face_bin_range(const int *__restrict__ gtri, const double *__restrict__ xy, long long f,
                                               const LayerGrid &g, int &bx0, int &bx1, int &by0, int &by1) {
    const long long a = gtri[3 * f], b = gtri[3 * f + 1], c = gtri[3 * f + 2];
    const double xa = xy[2 * a], ya = xy[2 * a + 1], xb = xy[2 * b], yb = xy[2 * b + 1], xc = xy[2 * c], yc = xy[2 * c + 1];
    const double lx = fmin(fmin(xa, xb), xc), hx = fmax(fmax(xa, xb), xc);
    const double ly = fmin(fmin(ya, yb), yc), hy = fmax(fmax(ya, yb), yc);
    const double S = fmax(hx - lx, hy - ly);
    if (!(S > 0.0)) return false;                 // three corners in one point: all sides are exact zeros, it contains nothing
    const double area2 = fabs(orient(xa, ya, xb, yb, xc, yc)) - 16.0 * DBL_EPSILON * S * S;       // a lower bound of 2 A
    if (!(area2 >= 256.0 * DBL_EPSILON * S * S)) {
        bx0 = by0 = 0;
        bx1 = g.nbx - 1;
        by1 = g.nby - 1;
        return true;
    }
    const double m = 128.0 * DBL_EPSILON * S * S * S / area2;
    bx0 = bin_of(lx - m, g.x0, g.sx, g.nbx);
    bx1 = bin_of(hx + m, g.x0, g.sx, g.nbx);
    by0 = bin_of(ly - m, g.y0, g.sy, g.nby);
    by1 = bin_of(hy + m, g.y0, g.sy, g.nby);
    return true;
}

// global corners of every face, checked once: gtri[f] = mesh_voff[m] + tri[f]
__global__ __launch_bounds__(256) void sampler_corners_kernel(long long n_tri, const int *__restrict__ tri, int n_mesh,
                                                              const long long *__restrict__ mesh_voff,
                                                              const long long *__restrict__ mesh_toff, int *__restrict__ gtri,
                                                              int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(mesh_toff, n_mesh, t);
    const long long v0 = mesh_voff[m], nv = mesh_voff[m + 1] - v0;
    for (int k = 0; k < 3; ++k) {
        const int l = tri[3 * t + k];
        if (l < 0 || l >= nv) {
            *(volatile int *)err = 1;
            gtri[3 * t + k] = (int)v0;
        } else {
            gtri[3 * t + k] = (int)(v0 + l);
        }
    }
}

// FILL = false: count[bin] += 1 for every bin of every face; FILL = true: the face takes the next place of each of its bins
// (count is then the cursor, a copy of the offsets).  Integer atomics; nothing depends on the order inside a bin.
template <bool FILL>
__global__ __launch_bounds__(256) void sampler_bin_kernel(long long n_tri, const int *__restrict__ gtri,
                                                          const double *__restrict__ xy, int n_mesh,
                                                          const long long *__restrict__ mesh_toff,
                                                          const int *__restrict__ mesh_layer,
                                                          const LayerGrid *__restrict__ grids, int *__restrict__ count,
                                                          int *__restrict__ bin_face) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_tri) return;
    const int layer = mesh_layer[find_segment(mesh_toff, n_mesh, f)];
    if (layer < 0) return;                        // a mesh the index leaves out (stack.hip: a layer no pair names)
    const LayerGrid g = grids[layer];
    int bx0, bx1, by0, by1;
    if (!face_bin_range(gtri, xy, f, g, bx0, bx1, by0, by1)) return;
    for (int by = by0; by <= by1; ++by)
        for (int bx = bx0; bx <= bx1; ++bx) {
            const int at = atomicAdd(&count[g.bin0 + (long long)by * g.nbx + bx], 1);
            if (FILL) bin_face[at] = (int)f;
        }
}

// One thread per query: the bin of q, the candidates of that bin, the owner, then the owner's values.  RASTER: q is the
// centre of pixel (row j, column i) of `r`, formed here; otherwise q = q_xy[idx].  Outside the copper: face -1, NaN.
//   potential   s = (o_a + o_b) + o_c;  V = ((o_a / s) V_a + (o_b / s) V_b) + (o_c / s) V_c     (o_a: the side of the edge
//               opposite corner a = tri[0], and so on: DESIGN.md)
//   J, p        current_face_kernel's and power_density_kernel's arithmetic on the owner, corners as (tri[2], tri[0], tri[1])
template <bool RASTER>
__global__ __launch_bounds__(256) void sample_kernel(const LayerGrid g, const int *__restrict__ bin_off,
                                                     const int *__restrict__ bin_face, const int *__restrict__ gtri,
                                                     const double *__restrict__ xy, int n_mesh,
                                                     const long long *__restrict__ mesh_toff, const double *__restrict__ sigma,
                                                     const double *__restrict__ V, long long n, const double *__restrict__ q_xy,
                                                     const RasterSpec r, int *__restrict__ face_out, double *__restrict__ v_out,
                                                     double *__restrict__ j_out, double *__restrict__ p_out,
                                                     unsigned long long *__restrict__ tested) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    unsigned long long n_tested = 0;
    if (live) {
        double qx, qy;
        if (RASTER) {
            const long long j = idx / r.width, i = idx - j * r.width;
            qx = r.x0 + ((double)i + 0.5) * r.dx;
            qy = r.y0 + ((double)j + 0.5) * r.dy;
        } else {
            qx = q_xy[2 * idx];
            qy = q_xy[2 * idx + 1];
        }
        double wa, wb, wc;
        const int owner = locate_owner(g, bin_off, bin_face, gtri, xy, qx, qy, wa, wb, wc, n_tested);
        int face = -1;
        double v = NAN, jx = NAN, jy = NAN, p = NAN;
        if (owner != kNoOwner) {
            face = owner;
            const long long a = gtri[3 * (long long)owner], b = gtri[3 * (long long)owner + 1], c = gtri[3 * (long long)owner + 2];
            const double va = V[a], vb = V[b], vc = V[c];
            const double s = (wa + wb) + wc;
            v = ((wa / s) * va + (wb / s) * vb) + (wc / s) * vc;
            double gx, gy;
            face_gradient_of(xy[2 * c], xy[2 * c + 1], xy[2 * a], xy[2 * a + 1], xy[2 * b], xy[2 * b + 1], vc, va, vb, gx, gy);
            const double sg = sigma[find_segment(mesh_toff, n_mesh, owner)];
            jx = -sg * gx;
            jy = -sg * gy;
            p = face_power_of(gx, gy, sg);
        }
        face_out[idx] = face;
        v_out[idx] = v;
        j_out[2 * idx] = jx;
        j_out[2 * idx + 1] = jy;
        p_out[idx] = p;
    }
    // candidates tested by this call (padne_sampler_stats): one integer atomic per wave
    for (int off = 32; off > 0; off >>= 1) n_tested += __shfl_down(n_tested, off, 64);
    if ((threadIdx.x & 63) == 0 && n_tested) atomicAdd(tested, n_tested);
}

// ---- thermal images: a block of fields read out at one located point ("Thermal images") -----------------------
constexpr int kMaxSampleFields = 256;
constexpr long long kMaxSampleValues = 1LL << 28;     // n_field x samples of one call that wants every field

// The (value, pixel) top of a 256-thread workgroup, in error.hpp's order: down each wave by halving strides, then waves 0 to
// 3 by thread 0, which alone holds the result.  red_*: 4 entries of shared memory each, free again after the caller's next
// barrier
__device__ __forceinline__ void field_block_top(double &v, long long &pix, double *red_v, long long *red_p) {
    error_wave_top(v, pix);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = v;
        red_p[threadIdx.x >> 6] = pix;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) error_merge(v, pix, red_v[w], red_p[w]);
}

// One thread per query: the owner ONCE, its weights and corners kept in registers, then every field of the field-major
// block T[n_field][n_vert] at it, stored field-major to t_out[n_field][n] and q_out[n_field][n][2] (either may be null:
// not computed, not stored), and the sequential maximum over the fields to hot_out / hot_field_out (field 0 first,
// replaced on strictly greater).  Outside the copper: face -1, NaN, field -1.
//   T_f   s = (o_a + o_b) + o_c;  ((o_a / s) T_f[a] + (o_b / s) T_f[b]) + (o_c / s) T_f[c]: sample_kernel's potential
//   q_f   -kappa_m grad T_f with sample_kernel's gradient, corners as (tri[2], tri[0], tri[1])
// RASTER: the pixel centres are formed here, and every workgroup leaves the top of its 256 pixels per slot (the fields, then
// the hottest) in tile_v / tile_p[slot][tile]: the larger value, the lower pixel on a tie, (-inf, kErrNoFace) for a
// workgroup without a pixel on copper.  No floating-point atomics anywhere.
template <bool RASTER>
__global__ __launch_bounds__(256) void sample_fields_kernel(const LayerGrid g, const int *__restrict__ bin_off,
                                                            const int *__restrict__ bin_face, const int *__restrict__ gtri,
                                                            const double *__restrict__ xy, int n_mesh,
                                                            const long long *__restrict__ mesh_toff,
                                                            const double *__restrict__ kappa, const double *__restrict__ T,
                                                            int n_field, long long n_vert, long long n,
                                                            const double *__restrict__ q_xy, const RasterSpec r,
                                                            int *__restrict__ face_out, double *__restrict__ t_out,
                                                            double *__restrict__ q_out, double *__restrict__ hot_out,
                                                            int *__restrict__ hot_field_out, double *__restrict__ tile_v,
                                                            long long *__restrict__ tile_p,
                                                            unsigned long long *__restrict__ tested) {
    __shared__ double red_v[2][4];
    __shared__ long long red_p[2][4];
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    unsigned long long n_tested = 0;
    bool has = false;
    long long a = 0, b = 0, c = 0;
    double la = 0.0, lb = 0.0, lc = 0.0, kap = 0.0;
    double xa = 0.0, ya = 0.0, xb = 0.0, yb = 0.0, xc = 0.0, yc = 0.0;
    if (live) {
        double qx, qy;
        if (RASTER) {
            const long long j = idx / r.width, i = idx - j * r.width;
            qx = r.x0 + ((double)i + 0.5) * r.dx;
            qy = r.y0 + ((double)j + 0.5) * r.dy;
        } else {
            qx = q_xy[2 * idx];
            qy = q_xy[2 * idx + 1];
        }
        double wa, wb, wc;
        const int owner = locate_owner(g, bin_off, bin_face, gtri, xy, qx, qy, wa, wb, wc, n_tested);
        has = owner != kNoOwner;
        if (has) {
            a = gtri[3 * (long long)owner];
            b = gtri[3 * (long long)owner + 1];
            c = gtri[3 * (long long)owner + 2];
            const double s = (wa + wb) + wc;
            la = wa / s;
            lb = wb / s;
            lc = wc / s;
            if (q_out) {
                xa = xy[2 * a]; ya = xy[2 * a + 1];
                xb = xy[2 * b]; yb = xy[2 * b + 1];
                xc = xy[2 * c]; yc = xy[2 * c + 1];
                kap = kappa[find_segment(mesh_toff, n_mesh, owner)];
            }
        }
        face_out[idx] = has ? owner : -1;
    }
    double hot = NAN;
    int hot_field = -1;
    const long long tile = blockIdx.x, n_tile = gridDim.x;
    for (int f = 0; f < n_field; ++f) {
        double t = NAN, qx = NAN, qy = NAN;
        if (has) {
            const double *__restrict__ Tf = T + (long long)f * n_vert;
            const double ta = Tf[a], tb = Tf[b], tc = Tf[c];
            t = (la * ta + lb * tb) + lc * tc;
            if (f == 0 || t > hot) {
                hot = t;
                hot_field = f;
            }
            if (q_out) {
                double gx, gy;
                face_gradient_of(xc, yc, xa, ya, xb, yb, tc, ta, tb, gx, gy);
                qx = -kap * gx;
                qy = -kap * gy;
            }
        }
        if (live) {
            if (t_out) t_out[(long long)f * n + idx] = t;
            if (q_out) {
                q_out[2 * ((long long)f * n + idx)] = qx;
                q_out[2 * ((long long)f * n + idx) + 1] = qy;
            }
        }
        if (RASTER) {
            double v = has ? t : -INFINITY;
            long long pix = has ? idx : kErrNoFace;
            field_block_top(v, pix, red_v[f & 1], red_p[f & 1]);
            if (threadIdx.x == 0) {
                tile_v[(long long)f * n_tile + tile] = v;
                tile_p[(long long)f * n_tile + tile] = pix;
            }
        }
    }
    if (live) {
        hot_out[idx] = hot;
        hot_field_out[idx] = hot_field;
    }
    if (RASTER) {
        double v = has ? hot : -INFINITY;
        long long pix = has ? idx : kErrNoFace;
        field_block_top(v, pix, red_v[n_field & 1], red_p[n_field & 1]);
        if (threadIdx.x == 0) {
            tile_v[(long long)n_field * n_tile + tile] = v;
            tile_p[(long long)n_field * n_tile + tile] = pix;
        }
    }
    for (int off = 32; off > 0; off >>= 1) n_tested += __shfl_down(n_tested, off, 64);
    if ((threadIdx.x & 63) == 0 && n_tested) atomicAdd(tested, n_tested);
}

// A workgroup per slot folds the slot's tiles: a thread takes tiles threadIdx.x, + 256, ... in order, then the workgroup's
// top.  top_p = -1 and top_v = -inf for a raster without a pixel on copper
__global__ __launch_bounds__(256) void sample_fields_fold_kernel(long long n_tile, const double *__restrict__ tile_v,
                                                                 const long long *__restrict__ tile_p,
                                                                 double *__restrict__ top_v, long long *__restrict__ top_p) {
    __shared__ double red_v[4];
    __shared__ long long red_p[4];
    const long long slot = blockIdx.x;
    double v = -INFINITY;
    long long pix = kErrNoFace;
    for (long long i = threadIdx.x; i < n_tile; i += 256) error_merge(v, pix, tile_v[slot * n_tile + i], tile_p[slot * n_tile + i]);
    field_block_top(v, pix, red_v, red_p);
    if (threadIdx.x == 0) {
        top_v[slot] = v;
        top_p[slot] = pix == kErrNoFace ? -1 : pix;
    }
}

}  // namespace padne

using namespace padne;

struct padne_sampler {
    padne_ctx *owner = nullptr;
    int64_t n_vert = 0, n_tri = 0;
    int32_t n_mesh = 0, n_layer = 0;
    // device (the owner's pool)
    double *xy = nullptr, *sigma = nullptr, *V = nullptr;
    int *gtri = nullptr, *mesh_layer = nullptr, *bin_off = nullptr, *bin_face = nullptr;
    long long *toff = nullptr;
    unsigned long long *tested = nullptr;
    double *T = nullptr, *kappa = nullptr;        // the field block [n_field][n_vert] and kappa[n_mesh] of padne_sampler_set_fields
    int32_t n_field = 0;
    // host
    std::vector<LayerGrid> grid;
    std::vector<int64_t> layer_faces, layer_entries;
    int64_t last_candidates = 0, last_queries = 0;
    double upload_seconds = 0, build_seconds = 0, last_kernel_seconds = 0;
};

static void sampler_free(padne_sampler *s) {
    if (s == nullptr) return;
    void *blocks[] = {s->xy, s->sigma, s->V, s->gtri, s->mesh_layer, s->bin_off, s->bin_face, s->toff, s->tested, s->T, s->kappa};
    for (void *p : blocks)
        if (p) pool_free(s->owner, p);
    delete s;
}

template <typename T> static int sampler_alloc(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

static double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the grid of a layer with n_faces faces in the box [lo, hi]: `bins` bins in all, as square as the box allows
static void choose_grid(LayerGrid &g, const double lo[2], const double hi[2], int64_t bins) {
    const double w = hi[0] - lo[0], h = hi[1] - lo[1];
    g.nbx = g.nby = 1;
    if (bins > 1 && w > 0 && h > 0) {
        g.nbx = (int)std::min<double>(kMaxBinsPerSide, std::max(1.0, std::floor(std::sqrt((double)bins * w / h) + 0.5)));
        g.nby = (int)std::min<double>(kMaxBinsPerSide, std::max(1.0, std::floor((double)bins / g.nbx + 0.5)));
    }
}

static void set_scale(LayerGrid &g, const double lo[2], const double hi[2]) {
    g.x0 = lo[0];
    g.y0 = lo[1];
    g.sx = g.nbx > 1 ? g.nbx / (hi[0] - lo[0]) : 0.0;
    g.sy = g.nby > 1 ? g.nby / (hi[1] - lo[1]) : 0.0;
}

int padne::locate_global_corners(padne_ctx *ctx, long long n_tri, const int *tri, int n_mesh, const long long *mesh_voff,
                                 const long long *mesh_toff, int *gtri, int *err_dev) {
    if (n_tri > 0) {
        hipLaunchKernelGGL(sampler_corners_kernel, dim3(nblk(n_tri)), dim3(256), 0, ctx->stream, n_tri, tri, n_mesh, mesh_voff,
                           mesh_toff, gtri, err_dev);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return PADNE_OK;
}

int padne::locate_build_bins(padne_ctx *ctx, int n_layer, const double *lo, const double *hi, int64_t bins_hint,
                             const std::vector<int64_t> &layer_faces, long long n_tri, const int *gtri, const double *xy,
                             int n_mesh, const long long *mesh_toff, const int *mesh_layer, std::vector<LayerGrid> &grid,
                             std::vector<int64_t> &layer_entries, int **bin_off, int **bin_face) {
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    struct PoolBlock {      // the counters of the round under way
        padne_ctx *ctx;
        void *p;
        ~PoolBlock() { if (p) pool_free(ctx, p); }
    } count{ctx, nullptr};
    LayerGrid *d_grid = nullptr;
    PADNE_TRY(sc.alloc(&d_grid, (size_t)n_layer));
    for (int l = 0; l < n_layer; ++l)
        choose_grid(grid[l], &lo[2 * l], &hi[2 * l], bins_hint > 0 ? bins_hint : std::max<int64_t>(1, layer_faces[l] / 2));
    for (;;) {
        long long n_bins = 0;
        for (int l = 0; l < n_layer; ++l) {
            set_scale(grid[l], &lo[2 * l], &hi[2 * l]);
            grid[l].bin0 = n_bins;
            n_bins += (long long)grid[l].nbx * grid[l].nby;
        }
        PADNE_REQUIRE(n_bins < (1LL << 30), "too many bins");
        if (*bin_off) pool_free(ctx, *bin_off);
        *bin_off = nullptr;
        PADNE_TRY(sampler_alloc(ctx, bin_off, (size_t)n_bins + 1));
        if (count.p) pool_free(ctx, count.p);
        count.p = pool_alloc(ctx, sizeof(int) * (size_t)(n_bins + 1));
        if (count.p == nullptr) return PADNE_E_NOMEM;
        int *d_count = (int *)count.p;
        PADNE_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)(n_bins + 1), st));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_grid, grid.data(), sizeof(LayerGrid) * (size_t)n_layer, hipMemcpyHostToDevice, st));
        if (n_tri > 0) {
            hipLaunchKernelGGL(sampler_bin_kernel<false>, dim3(nblk(n_tri)), dim3(256), 0, st, n_tri, gtri, xy,
                               n_mesh, mesh_toff, mesh_layer, d_grid, d_count, (int *)nullptr);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        bool negative = false;
        int64_t total = 0;
        PADNE_TRY(exclusive_scan_i32_flagged(ctx, d_count, *bin_off, n_bins, &total, &negative));
        if (negative || total >= (1LL << 31)) {       // a count wrapped: only far finer than kListBound allows; coarsen
            total = -1;
        }
        std::vector<int> first(n_layer + 1, 0);
        bool again = false;
        if (total >= 0) {
            for (int l = 0; l < n_layer; ++l)
                PADNE_HIP_CHECK(hipMemcpyAsync(&first[l], *bin_off + grid[l].bin0, sizeof(int), hipMemcpyDeviceToHost, st));
            PADNE_HIP_CHECK(hipStreamSynchronize(st));
            first[n_layer] = (int)total;
        }
        for (int l = 0; l < n_layer; ++l) {
            LayerGrid &g = grid[l];
            layer_entries[l] = total >= 0 ? (int64_t)first[l + 1] - first[l] : -1;
            const bool too_long = total < 0 || layer_entries[l] > kListBound * layer_faces[l];
            if (too_long && (g.nbx > 1 || g.nby > 1)) {
                g.nbx = (g.nbx + 1) / 2;
                g.nby = (g.nby + 1) / 2;
                again = true;
            }
        }
        if (again) continue;
        PADNE_REQUIRE(total >= 0, "the face lists do not fit 32-bit offsets");
        PADNE_TRY(sampler_alloc(ctx, bin_face, (size_t)total));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_count, *bin_off, sizeof(int) * (size_t)n_bins, hipMemcpyDeviceToDevice, st));
        if (n_tri > 0) {
            hipLaunchKernelGGL(sampler_bin_kernel<true>, dim3(nblk(n_tri)), dim3(256), 0, st, n_tri, gtri, xy,
                               n_mesh, mesh_toff, mesh_layer, d_grid, d_count, *bin_face);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        PADNE_HIP_CHECK(hipStreamSynchronize(st));
        break;
    }
    return PADNE_OK;
}

extern "C" int padne_sampler_create(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri,
                                    const int32_t *tri_host, int32_t n_mesh, const int64_t *mesh_vertex_offset,
                                    const int64_t *mesh_tri_offset, const int32_t *mesh_layer, const double *conductance,
                                    int32_t n_layer, const double *potential_host, int64_t bins_hint, padne_sampler **out) {
    PADNE_REQUIRE(ctx && out, "null argument");
    *out = nullptr;
    PADNE_REQUIRE(n_vert >= 0 && n_tri >= 0 && n_mesh >= 0 && n_layer >= 1 && bins_hint >= 0, "negative size or no layer");
    PADNE_REQUIRE(n_vert < (1LL << 31) && n_tri < (1LL << 27), "a sampler takes fewer than 2^31 vertices and 2^27 faces");
    PADNE_REQUIRE(mesh_vertex_offset && mesh_tri_offset, "null argument");
    PADNE_REQUIRE(n_mesh == 0 || (mesh_layer && conductance), "null argument");
    PADNE_REQUIRE((n_vert == 0 || (xy_host && potential_host)) && (n_tri == 0 || tri_host), "null argument");
    PADNE_REQUIRE(mesh_vertex_offset[0] == 0 && mesh_tri_offset[0] == 0, "offset tables must start at 0");
    PADNE_REQUIRE(mesh_vertex_offset[n_mesh] == n_vert && mesh_tri_offset[n_mesh] == n_tri, "offset tables");
    for (int32_t m = 0; m < n_mesh; ++m) {
        PADNE_REQUIRE(mesh_vertex_offset[m] <= mesh_vertex_offset[m + 1] && mesh_tri_offset[m] <= mesh_tri_offset[m + 1],
                      "offset tables not monotone");
        PADNE_REQUIRE(mesh_layer[m] >= 0 && mesh_layer[m] < n_layer, "mesh layer out of range");
    }
    for (int64_t i = 0; i < 2 * n_vert; ++i) PADNE_REQUIRE(std::isfinite(xy_host[i]), "vertex coordinates must be finite");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const auto t0 = std::chrono::steady_clock::now();
    padne_sampler *s = new padne_sampler;
    s->owner = ctx;
    s->n_vert = n_vert;
    s->n_tri = n_tri;
    s->n_mesh = n_mesh;
    s->n_layer = n_layer;
    s->grid.resize(n_layer);
    s->layer_faces.assign(n_layer, 0);
    s->layer_entries.assign(n_layer, 0);
    struct Guard {      // an error path hands everything back
        padne_sampler *s;
        ~Guard() { sampler_free(s); }
    } guard{s};
    std::vector<long long> toff(mesh_tri_offset, mesh_tri_offset + n_mesh + 1), voff(mesh_vertex_offset, mesh_vertex_offset + n_mesh + 1);
    Scratch sc(ctx);
    int *d_tri = nullptr, *d_err = nullptr;
    long long *d_voff = nullptr;
    PADNE_TRY(sampler_alloc(ctx, &s->xy, (size_t)n_vert * 2));
    PADNE_TRY(sampler_alloc(ctx, &s->V, (size_t)n_vert));
    PADNE_TRY(sampler_alloc(ctx, &s->sigma, (size_t)n_mesh));
    PADNE_TRY(sampler_alloc(ctx, &s->gtri, (size_t)n_tri * 3));
    PADNE_TRY(sampler_alloc(ctx, &s->mesh_layer, (size_t)n_mesh));
    PADNE_TRY(sampler_alloc(ctx, &s->toff, (size_t)n_mesh + 1));
    PADNE_TRY(sampler_alloc(ctx, &s->tested, 1));
    PADNE_TRY(sc.alloc(&d_tri, (size_t)n_tri * 3));
    PADNE_TRY(sc.alloc(&d_voff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_err, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), st));
    PADNE_HIP_CHECK(hipMemcpyAsync(s->xy, xy_host, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(s->V, potential_host, sizeof(double) * (size_t)n_vert, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tri, tri_host, sizeof(int) * 3 * (size_t)n_tri, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(s->sigma, conductance, sizeof(double) * (size_t)n_mesh, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(s->mesh_layer, mesh_layer, sizeof(int) * (size_t)n_mesh, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(s->toff, toff.data(), sizeof(long long) * (size_t)(n_mesh + 1), hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_voff, voff.data(), sizeof(long long) * (size_t)(n_mesh + 1), hipMemcpyHostToDevice, st));
    PADNE_TRY(locate_global_corners(ctx, (long long)n_tri, d_tri, (int)n_mesh, d_voff, s->toff, s->gtri, d_err));
    int h_err = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    if (h_err) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    s->upload_seconds = seconds_since(t0);

    // ---- the index: bounding box and grid of every layer, then count, scan, fill; coarsened while a layer's lists are
    // longer than kListBound entries per face
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<double> lo(2 * (size_t)n_layer, INFINITY), hi(2 * (size_t)n_layer, -INFINITY);
    for (int32_t m = 0; m < n_mesh; ++m) {
        const int l = mesh_layer[m];
        s->layer_faces[l] += mesh_tri_offset[m + 1] - mesh_tri_offset[m];
        for (int64_t v = mesh_vertex_offset[m]; v < mesh_vertex_offset[m + 1]; ++v)
            for (int k = 0; k < 2; ++k) {
                lo[2 * l + k] = std::min(lo[2 * l + k], xy_host[2 * v + k]);
                hi[2 * l + k] = std::max(hi[2 * l + k], xy_host[2 * v + k]);
            }
    }
    for (int l = 0; l < n_layer; ++l)
        if (!(lo[2 * l] <= hi[2 * l])) lo[2 * l] = lo[2 * l + 1] = hi[2 * l] = hi[2 * l + 1] = 0.0;      // a layer without vertices
    PADNE_TRY(locate_build_bins(ctx, (int)n_layer, lo.data(), hi.data(), bins_hint, s->layer_faces, (long long)n_tri, s->gtri, s->xy,
                                (int)n_mesh, s->toff, s->mesh_layer, s->grid, s->layer_entries, &s->bin_off, &s->bin_face));
    s->build_seconds = seconds_since(t1);
    guard.s = nullptr;
    *out = s;
    return PADNE_OK;
}

extern "C" int padne_sampler_destroy(padne_sampler *s) {
    if (s == nullptr) return PADNE_OK;
    if (s->owner) {
        (void)hipSetDevice(s->owner->device);
        (void)hipStreamSynchronize(s->owner->stream);
    }
    sampler_free(s);
    return PADNE_OK;
}

// the shared body of the two query entries: q_host != nullptr -> points, else the raster r
static int sampler_query(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *q_host, const RasterSpec &r,
                         int32_t *face_out, double *v_out, double *j_out, double *p_out) {
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    double *d_q = nullptr, *d_v = nullptr, *d_j = nullptr, *d_p = nullptr;
    int *d_face = nullptr;
    if (q_host) PADNE_TRY(sc.alloc(&d_q, (size_t)n * 2));
    PADNE_TRY(sc.alloc(&d_face, (size_t)n));
    PADNE_TRY(sc.alloc(&d_v, (size_t)n));
    PADNE_TRY(sc.alloc(&d_j, (size_t)n * 2));
    PADNE_TRY(sc.alloc(&d_p, (size_t)n));
    PADNE_HIP_CHECK(hipMemsetAsync(s->tested, 0, sizeof(unsigned long long), st));
    if (q_host) PADNE_HIP_CHECK(hipMemcpyAsync(d_q, q_host, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipEventRecord(ctx->ev0, st));
    if (q_host)
        hipLaunchKernelGGL(sample_kernel<false>, dim3(nblk(n)), dim3(256), 0, st, s->grid[layer], s->bin_off, s->bin_face, s->gtri,
                           s->xy, (int)s->n_mesh, s->toff, s->sigma, s->V, (long long)n, d_q, r, d_face, d_v, d_j, d_p, s->tested);
    else
        hipLaunchKernelGGL(sample_kernel<true>, dim3(nblk(n)), dim3(256), 0, st, s->grid[layer], s->bin_off, s->bin_face, s->gtri,
                           s->xy, (int)s->n_mesh, s->toff, s->sigma, s->V, (long long)n, (const double *)nullptr, r, d_face, d_v,
                           d_j, d_p, s->tested);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipEventRecord(ctx->ev1, st));
    unsigned long long tested = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&tested, s->tested, sizeof(tested), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(face_out, d_face, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(v_out, d_v, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(j_out, d_j, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(p_out, d_p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.0f;
    PADNE_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    s->last_kernel_seconds = 1e-3 * ms;
    s->last_candidates = (int64_t)tested;
    s->last_queries = n;
    return PADNE_OK;
}

static int sampler_query_checks(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const void *a, const void *b,
                                const void *c, const void *d) {
    PADNE_REQUIRE(ctx && s, "null argument");
    PADNE_REQUIRE(s->owner == ctx, "the sampler belongs to another context");
    PADNE_REQUIRE(layer >= 0 && layer < s->n_layer, "layer out of range");
    PADNE_REQUIRE(n >= 0 && n <= kMaxSamples, "at most 2^26 samples in one call");
    PADNE_REQUIRE(n == 0 || (a && b && c && d), "null argument");
    return PADNE_OK;
}

extern "C" int padne_sampler_points(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *xy_host,
                                    int32_t *face_out, double *v_out, double *j_out, double *p_out) {
    PADNE_TRY(sampler_query_checks(ctx, s, layer, n, face_out, v_out, j_out, p_out));
    PADNE_REQUIRE(n == 0 || xy_host, "null argument");
    for (int64_t i = 0; i < 2 * n; ++i) PADNE_REQUIRE(std::isfinite(xy_host[i]), "query points must be finite");
    if (n == 0) {
        s->last_candidates = s->last_queries = 0;
        s->last_kernel_seconds = 0;
        return PADNE_OK;
    }
    return sampler_query(ctx, s, layer, n, xy_host, RasterSpec{0, 0, 0, 0, 1}, face_out, v_out, j_out, p_out);
}

extern "C" int padne_sampler_raster(padne_ctx *ctx, padne_sampler *s, int32_t layer, double x0, double y0, double dx, double dy,
                                    int64_t width, int64_t height, int32_t *face_out, double *v_out, double *j_out,
                                    double *p_out) {
    PADNE_REQUIRE(width >= 1 && height >= 1, "a raster has at least one pixel");
    PADNE_REQUIRE(width <= kMaxSamples && height <= kMaxSamples, "at most 2^26 samples in one call");
    PADNE_TRY(sampler_query_checks(ctx, s, layer, width * height, face_out, v_out, j_out, p_out));
    PADNE_REQUIRE(std::isfinite(x0) && std::isfinite(y0), "the raster's origin must be finite");
    PADNE_REQUIRE(std::isfinite(dx) && std::isfinite(dy) && dx > 0 && dy > 0, "the pixel size must be finite and positive");
    // the last pixel centre is the largest coordinate the kernel forms
    PADNE_REQUIRE(std::isfinite(x0 + ((double)(width - 1) + 0.5) * dx) && std::isfinite(y0 + ((double)(height - 1) + 0.5) * dy),
                  "the raster's pixel centres must be finite");
    return sampler_query(ctx, s, layer, width * height, nullptr, RasterSpec{x0, y0, dx, dy, (long long)width}, face_out, v_out,
                         j_out, p_out);
}

extern "C" int padne_sampler_stats(const padne_sampler *s, int32_t layer, int64_t *counts_out, double *seconds_out) {
    PADNE_REQUIRE(s && counts_out && seconds_out, "null argument");
    PADNE_REQUIRE(layer >= 0 && layer < s->n_layer, "layer out of range");
    counts_out[0] = s->grid[layer].nbx;
    counts_out[1] = s->grid[layer].nby;
    counts_out[2] = s->layer_entries[layer];
    counts_out[3] = s->layer_faces[layer];
    counts_out[4] = s->last_candidates;
    counts_out[5] = s->last_queries;
    seconds_out[0] = s->upload_seconds;
    seconds_out[1] = s->build_seconds;
    seconds_out[2] = s->last_kernel_seconds;
    return PADNE_OK;
}

// ---- thermal images ------------------------------------------------------------------------------------------------------

extern "C" int padne_sampler_set_fields(padne_ctx *ctx, padne_sampler *s, int32_t n_field, const double *fields_host,
                                        const double *kappa) {
    PADNE_REQUIRE(ctx && s, "null argument");
    PADNE_REQUIRE(s->owner == ctx, "the sampler belongs to another context");
    PADNE_REQUIRE(n_field >= 0 && n_field <= kMaxSampleFields, "a sampler takes at most 256 fields");
    PADNE_REQUIRE(n_field == 0 || s->n_vert == 0 || fields_host, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double *T = nullptr, *kap = nullptr;
    if (n_field > 0) {
        PADNE_TRY(sampler_alloc(ctx, &T, (size_t)n_field * (size_t)s->n_vert));
        if (kappa && sampler_alloc(ctx, &kap, (size_t)s->n_mesh) != PADNE_OK) {
            pool_free(ctx, T);
            return PADNE_E_NOMEM;
        }
        hipError_t e = hipSuccess;
        if (s->n_vert > 0)
            e = hipMemcpyAsync(T, fields_host, sizeof(double) * (size_t)n_field * (size_t)s->n_vert, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && kap && s->n_mesh > 0)
            e = hipMemcpyAsync(kap, kappa, sizeof(double) * (size_t)s->n_mesh, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            pool_free(ctx, T);
            if (kap) pool_free(ctx, kap);
            PADNE_HIP_CHECK(e);
        }
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(st));      // nothing queued reads the block that leaves
    if (s->T) pool_free(ctx, s->T);
    if (s->kappa) pool_free(ctx, s->kappa);
    s->T = T;
    s->kappa = kap;
    s->n_field = n_field;
    return PADNE_OK;
}

static int sampler_field_checks(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const void *face_out,
                                const void *t_out, const void *q_out, const void *hot_out, const void *hot_field_out) {
    PADNE_REQUIRE(ctx && s, "null argument");
    PADNE_REQUIRE(s->owner == ctx, "the sampler belongs to another context");
    PADNE_REQUIRE(s->n_field > 0, "the sampler has no fields: padne_sampler_set_fields comes first");
    PADNE_REQUIRE(q_out == nullptr || s->kappa, "the heat flux needs the sheet conductances kappa");
    PADNE_REQUIRE(layer >= 0 && layer < s->n_layer, "layer out of range");
    PADNE_REQUIRE(n >= 0 && n <= kMaxSamples, "at most 2^26 samples in one call");
    PADNE_REQUIRE((t_out == nullptr && q_out == nullptr) || (long long)s->n_field * n <= kMaxSampleValues,
                  "at most 2^28 values (fields x samples) in one call that returns every field");
    PADNE_REQUIRE(n == 0 || (face_out && hot_out && hot_field_out), "null argument");
    return PADNE_OK;
}

// the shared body of the two field entries: q_host != nullptr -> points, else the raster r with its tops
static int sampler_field_query(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *q_host,
                               const RasterSpec &r, int32_t *face_out, double *t_out, double *q_out, double *hot_out,
                               int32_t *hot_field_out, double *top_out, int64_t *top_pixel_out) {
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    const size_t F = (size_t)s->n_field, n_tile = nblk(n);
    double *d_q = nullptr, *d_t = nullptr, *d_flux = nullptr, *d_hot = nullptr, *d_tile_v = nullptr, *d_top_v = nullptr;
    long long *d_tile_p = nullptr, *d_top_p = nullptr;
    int *d_face = nullptr, *d_hot_field = nullptr;
    if (q_host) PADNE_TRY(sc.alloc(&d_q, (size_t)n * 2));
    PADNE_TRY(sc.alloc(&d_face, (size_t)n));
    if (t_out) PADNE_TRY(sc.alloc(&d_t, F * (size_t)n));
    if (q_out) PADNE_TRY(sc.alloc(&d_flux, F * (size_t)n * 2));
    PADNE_TRY(sc.alloc(&d_hot, (size_t)n));
    PADNE_TRY(sc.alloc(&d_hot_field, (size_t)n));
    if (!q_host) {
        PADNE_TRY(sc.alloc(&d_tile_v, (F + 1) * n_tile));
        PADNE_TRY(sc.alloc(&d_tile_p, (F + 1) * n_tile));
        PADNE_TRY(sc.alloc(&d_top_v, F + 1));
        PADNE_TRY(sc.alloc(&d_top_p, F + 1));
    }
    PADNE_HIP_CHECK(hipMemsetAsync(s->tested, 0, sizeof(unsigned long long), st));
    if (q_host) PADNE_HIP_CHECK(hipMemcpyAsync(d_q, q_host, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    PADNE_HIP_CHECK(hipEventRecord(ctx->ev0, st));
    if (q_host) {
        hipLaunchKernelGGL(sample_fields_kernel<false>, dim3(n_tile), dim3(256), 0, st, s->grid[layer], s->bin_off, s->bin_face,
                           s->gtri, s->xy, (int)s->n_mesh, s->toff, s->kappa, s->T, (int)s->n_field, (long long)s->n_vert,
                           (long long)n, d_q, r, d_face, d_t, d_flux, d_hot, d_hot_field, (double *)nullptr,
                           (long long *)nullptr, s->tested);
        PADNE_HIP_CHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(sample_fields_kernel<true>, dim3(n_tile), dim3(256), 0, st, s->grid[layer], s->bin_off, s->bin_face,
                           s->gtri, s->xy, (int)s->n_mesh, s->toff, s->kappa, s->T, (int)s->n_field, (long long)s->n_vert,
                           (long long)n, (const double *)nullptr, r, d_face, d_t, d_flux, d_hot, d_hot_field, d_tile_v,
                           d_tile_p, s->tested);
        PADNE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(sample_fields_fold_kernel, dim3(F + 1), dim3(256), 0, st, (long long)n_tile, d_tile_v, d_tile_p,
                           d_top_v, d_top_p);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipEventRecord(ctx->ev1, st));
    unsigned long long tested = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&tested, s->tested, sizeof(tested), hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(face_out, d_face, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (t_out) PADNE_HIP_CHECK(hipMemcpyAsync(t_out, d_t, sizeof(double) * F * (size_t)n, hipMemcpyDeviceToHost, st));
    if (q_out) PADNE_HIP_CHECK(hipMemcpyAsync(q_out, d_flux, sizeof(double) * 2 * F * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(hot_out, d_hot, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    PADNE_HIP_CHECK(hipMemcpyAsync(hot_field_out, d_hot_field, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (!q_host) {
        static_assert(sizeof(long long) == sizeof(int64_t), "the tops' pixels are copied as they are");
        PADNE_HIP_CHECK(hipMemcpyAsync(top_out, d_top_v, sizeof(double) * (F + 1), hipMemcpyDeviceToHost, st));
        PADNE_HIP_CHECK(hipMemcpyAsync(top_pixel_out, d_top_p, sizeof(int64_t) * (F + 1), hipMemcpyDeviceToHost, st));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.0f;
    PADNE_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    s->last_kernel_seconds = 1e-3 * ms;
    s->last_candidates = (int64_t)tested;
    s->last_queries = n;
    return PADNE_OK;
}

extern "C" int padne_sampler_field_points(padne_ctx *ctx, padne_sampler *s, int32_t layer, int64_t n, const double *xy_host,
                                          int32_t *face_out, double *t_out, double *q_out, double *hot_out,
                                          int32_t *hot_field_out) {
    PADNE_TRY(sampler_field_checks(ctx, s, layer, n, face_out, t_out, q_out, hot_out, hot_field_out));
    PADNE_REQUIRE(n == 0 || xy_host, "null argument");
    for (int64_t i = 0; i < 2 * n; ++i) PADNE_REQUIRE(std::isfinite(xy_host[i]), "query points must be finite");
    if (n == 0) {
        s->last_candidates = s->last_queries = 0;
        s->last_kernel_seconds = 0;
        return PADNE_OK;
    }
    return sampler_field_query(ctx, s, layer, n, xy_host, RasterSpec{0, 0, 0, 0, 1}, face_out, t_out, q_out, hot_out,
                               hot_field_out, nullptr, nullptr);
}

extern "C" int padne_sampler_field_raster(padne_ctx *ctx, padne_sampler *s, int32_t layer, double x0, double y0, double dx,
                                          double dy, int64_t width, int64_t height, int32_t *face_out, double *t_out,
                                          double *q_out, double *hot_out, int32_t *hot_field_out, double *top_out,
                                          int64_t *top_pixel_out) {
    PADNE_REQUIRE(width >= 1 && height >= 1, "a raster has at least one pixel");
    PADNE_REQUIRE(width <= kMaxSamples && height <= kMaxSamples, "at most 2^26 samples in one call");
    PADNE_TRY(sampler_field_checks(ctx, s, layer, width * height, face_out, t_out, q_out, hot_out, hot_field_out));
    PADNE_REQUIRE(top_out && top_pixel_out, "null argument");
    PADNE_REQUIRE(std::isfinite(x0) && std::isfinite(y0), "the raster's origin must be finite");
    PADNE_REQUIRE(std::isfinite(dx) && std::isfinite(dy) && dx > 0 && dy > 0, "the pixel size must be finite and positive");
    PADNE_REQUIRE(std::isfinite(x0 + ((double)(width - 1) + 0.5) * dx) && std::isfinite(y0 + ((double)(height - 1) + 0.5) * dy),
                  "the raster's pixel centres must be finite");
    return sampler_field_query(ctx, s, layer, width * height, nullptr, RasterSpec{x0, y0, dx, dy, (long long)width}, face_out,
                               t_out, q_out, hot_out, hot_field_out, top_out, top_pixel_out);
}
