// Heat from components: footprints on a layer that dissipate watts ("Heat sources").  No reference counterpart.
//
// A source s is a layer, a polygon of n >= 3 vertices and a power p[c][s] >= 0 [W] per column c.  On the meshes the thermal
// handle's system keeps on the device:
//
//   centroid   cx = ((x1 + x2) + x3) / 3, cy likewise, the corners in the order of error_corners;
//   coverage   s covers face f when f belongs to a mesh of the source's layer and (cx, cy) lies inside the polygon by the
//              even-odd rule: the edge from (xj, yj) (the previous vertex, cyclic) to (xi, yi) crosses when
//              (yi > cy) != (yj > cy) and cx < (xj - xi) * (cy - yi) / (yj - yi) + xi; inside when the crossings are odd;
//   list       the covered faces in ascending global number; A_s = the sum of their areas (error_area) down the list in
//              tiles of 256: a tile is the workgroup sum of error.hpp, thread (i mod 256) adds tile i to its partial sum
//              front to back, and the 256 partial sums are joined by one more workgroup sum;
//   fallback   a source that covers no centroid (a footprint smaller than a face): q = the vertex mean of the polygon (the
//              coordinates summed in vertex order from 0.0, divided by n); its list is the one face that owns q among the
//              faces of the layer by the sampler's rule (locate.hpp: the containing face with the lowest global number);
//              none: the source lies on no copper the system keeps, which is refused;
//   load       b[c][v] = b[c][v] + acc, acc = the sum, from 0.0, over the faces f of v's list front to back and over the
//              sources s that cover f in ascending s, of ((area_f / A_s) * p[c][s]) / 3;
//   report     T_s[c] - ambient = the sum over the list, in the order of A_s, of (area_f / A_s) * mean[c][f], mean the
//              face mean of padne_thermal_report.
//
// The weights area_f / A_s of a source sum to 1: the load sums to p[c][s], and since K, the links and G annihilate
// constants the film loss still equals the heat put in.  The Joule array th->P is not touched.
//
// Kernels: streams and gathers bound by memory, workgroups of 256.  One workgroup per source walks the centroids of its
// layer's faces in ascending order with the polygon in LDS -- a count pass, the offsets on the host (one number per source),
// a fill pass that compacts every tile with wave ballots, so a list comes out ascending without a sort.  A bounding box
// in front of the edge loop: one compare per face outside it.  The box cannot change a decision: a centroid with cy
// outside [ymin, ymax) meets no edge that straddles it, and the box is widened in x by far more than the crossing abscissa
// can err, where an even number of straddling edges all cross or none does.  The face -> sources lists by count, scan and
// fill with one thread per face over the sources in ascending order.  No floating-point atomics: two calls give the same
// bits.  Compiled with -ffp-contract=off: the expressions round as written, tests/sources_ref.py reproduces them.
#include "locate.hpp"
#include "thermal.hpp"

#include <cmath>
#include <string>
#include <vector>

namespace padne {

constexpr int kSourceMaxVertices = 256;      // of a polygon: what the LDS image of the walk holds
constexpr int kSourceMaxCount = 4096;

void sources_free(padne_ctx *ctx, padne_sources *sr) {
    if (sr == nullptr) return;
    for (void *p : {(void *)sr->lptr, (void *)sr->lface, (void *)sr->fptr, (void *)sr->fsrc, (void *)sr->A, (void *)sr->face_area,
                    (void *)sr->power})
        if (p != nullptr) pool_free(ctx, p);
    delete sr;
}

// ---- coverage --------------------------------------------------------------------------------------------------------------
// the even-odd rule for the polygon poly[n][2] (LDS or global memory) behind its box (xlo, ylo, xhi, yhi)
__device__ __forceinline__ bool source_covers(const double *__restrict__ box, const double *poly, int n, double cx, double cy) {
    if (!(cy >= box[1] && cy < box[3] && cx >= box[0] && cx <= box[2])) return false;
    bool in = false;
    double xj = poly[2 * (n - 1)], yj = poly[2 * (n - 1) + 1];
    for (int i = 0; i < n; ++i) {
        const double xi = poly[2 * i], yi = poly[2 * i + 1];
        if ((yi > cy) != (yj > cy) && cx < (xj - xi) * (cy - yi) / (yj - yi) + xi) in = !in;
        xj = xi;
        yj = yi;
    }
    return in;
}

// area[t] = A_f and cen[t] = the centroid of every face.  One thread per face
__global__ __launch_bounds__(256) void sources_face_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                           const double *__restrict__ xy, const long long *__restrict__ voff,
                                                           const long long *__restrict__ toff, double *__restrict__ area,
                                                           double *__restrict__ cen, int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    long long g1, g2, g3;
    if (!error_corners(tri, voff, m, t, g1, g2, g3)) {
        *(volatile int *)err = 1;
        area[t] = 0.0;
        cen[2 * t] = cen[2 * t + 1] = 0.0;
        return;
    }
    const double x1 = xy[2 * g1], y1 = xy[2 * g1 + 1];
    const double x2 = xy[2 * g2], y2 = xy[2 * g2 + 1];
    const double x3 = xy[2 * g3], y3 = xy[2 * g3 + 1];
    area[t] = error_area(x1, y1, x2, y2, x3, y3);
    cen[2 * t] = ((x1 + x2) + x3) / 3;
    cen[2 * t + 1] = ((y1 + y2) + y3) / 3;
}

// Source s = blockIdx.x walks the faces of its layer's meshes in ascending order, 256 at a time.  FILL = false: count[s] =
// the faces it covers.  FILL = true: they are written from lptr[s] on, every tile compacted by the ballots of its four
// waves; a fallback source (owner[s] >= 0) writes its one face
template <bool FILL>
__global__ __launch_bounds__(256) void sources_walk_kernel(const int n_mesh, const int *__restrict__ mesh_layer,
                                                           const long long *__restrict__ toff, const double *__restrict__ cen,
                                                           const int *__restrict__ src_layer, const double *__restrict__ box,
                                                           const int *__restrict__ poly_ptr, const double *__restrict__ poly_xy,
                                                           const int *__restrict__ owner, const int *__restrict__ lptr,
                                                           int *__restrict__ lface, int *__restrict__ count) {
    __shared__ double poly[2 * kSourceMaxVertices];
    __shared__ int wave_n[4];
    const int s = blockIdx.x;
    if (FILL && owner[s] >= 0) {                             // (the same for the whole workgroup)
        if (threadIdx.x == 0) lface[lptr[s]] = owner[s];
        return;
    }
    const int p0 = poly_ptr[s], n = poly_ptr[s + 1] - p0;    // n <= kSourceMaxVertices: checked by the entry
    for (int i = threadIdx.x; i < 2 * n; i += 256) poly[i] = poly_xy[2 * (long long)p0 + i];
    __syncthreads();
    const int layer = src_layer[s], lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long base = FILL ? lptr[s] : 0;
    long long total = 0;
    for (int m = 0; m < n_mesh; ++m) {
        if (mesh_layer[m] != layer) continue;
        const long long t1 = toff[m + 1];
        for (long long t0 = toff[m]; t0 < t1; t0 += 256) {
            const long long t = t0 + threadIdx.x;
            const bool in = t < t1 && source_covers(box + 4 * s, poly, n, cen[2 * t], cen[2 * t + 1]);
            const unsigned long long ballot = __ballot(in);
            if (lane == 0) wave_n[w] = __popcll(ballot);
            __syncthreads();
            const int c0 = wave_n[0], c1 = wave_n[1], c2 = wave_n[2], c3 = wave_n[3];
            if (FILL && in) {
                const int before = (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + __popcll(ballot & ((1ull << lane) - 1ull));
                lface[base + total + before] = (int)t;
            }
            total += (c0 + c1) + (c2 + c3);
            __syncthreads();
        }
    }
    if (!FILL && threadIdx.x == 0) count[s] = (int)total;
}

// The fallback: for a source s = blockIdx.x that covers nothing (count[s] == 0), owner[s] = the face of its layer that owns
// q[s] by the rule of locate_owner -- the containing face with the lowest global number -- looked for among all faces of
// the layer; kNoOwner for none.  -1 for a source with a list
__global__ __launch_bounds__(256) void sources_owner_kernel(const int n_mesh, const int *__restrict__ mesh_layer,
                                                            const long long *__restrict__ toff, const long long *__restrict__ voff,
                                                            const int32_t *__restrict__ tri, const double *__restrict__ xy,
                                                            const int *__restrict__ src_layer, const int *__restrict__ count,
                                                            const double *__restrict__ q, int *__restrict__ owner) {
    __shared__ int red[4];
    const int s = blockIdx.x;
    if (count[s] != 0) {
        if (threadIdx.x == 0) owner[s] = -1;
        return;
    }
    const int layer = src_layer[s];
    const double qx = q[2 * s], qy = q[2 * s + 1];
    int best = kNoOwner;
    for (int m = 0; m < n_mesh; ++m) {
        if (mesh_layer[m] != layer) continue;
        const long long v0 = voff[m];
        for (long long t = toff[m] + threadIdx.x; t < toff[m + 1]; t += 256) {
            const int a = (int)(v0 + tri[3 * t]), b = (int)(v0 + tri[3 * t + 1]), c = (int)(v0 + tri[3 * t + 2]);
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
    if (threadIdx.x == 0) owner[s] = min(min(red[0], red[1]), min(red[2], red[3]));
}

// Sums down the list of source s = blockIdx.x in the order stated at the top.  TEMP = false: out[s] = A_s, the sum of the
// areas.  TEMP = true, column c = blockIdx.y: out[c][s] = the sum of (area_f / A_s) * mean[c][f], mean the face mean of
// thermal_report_face_kernel
template <bool TEMP>
__global__ __launch_bounds__(256) void sources_sum_kernel(const int n_source, const int *__restrict__ lptr,
                                                          const int *__restrict__ lface, const double *__restrict__ area,
                                                          const double *__restrict__ A, const int n_mesh,
                                                          const int32_t *__restrict__ tri, const long long *__restrict__ voff,
                                                          const long long *__restrict__ toff, const long long n_pot,
                                                          const double *__restrict__ theta, double *__restrict__ out) {
    __shared__ double red[4];
    const int s = blockIdx.x, lo = lptr[s], hi = lptr[s + 1];
    const double *th = TEMP ? theta + (long long)blockIdx.y * n_pot : nullptr;
    const double As = TEMP ? A[s] : 1.0;
    double part = 0.0;
    int tile = 0;
    for (long long i0 = lo; i0 < hi; i0 += 256, ++tile) {
        const long long i = i0 + threadIdx.x;
        double v = 0.0;
        if (i < hi) {
            const long long f = lface[i];
            if (TEMP) {
                long long g1 = 0, g2 = 0, g3 = 0;
                const bool ok = error_corners(tri, voff, find_segment(toff, n_mesh, f), f, g1, g2, g3);
                const double mean = ok ? ((th[g1] + th[g2]) + th[g3]) / 3 : 0.0;
                v = (area[f] / As) * mean;
            } else {
                v = area[f];
            }
        }
        v = error_wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if ((int)threadIdx.x == (tile & 255)) part = part + error_sum4(red);
        __syncthreads();
    }
    part = error_wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) out[(long long)blockIdx.y * n_source + s] = error_sum4(red);
}

// The sources of every face in ascending source number: a source with a list covers its centroid, a fallback source its
// owner.  FILL = false: count[t]; FILL = true: written from fptr[t] on.  One thread per face; the lanes of a wave read the
// same source at a time
template <bool FILL>
__global__ __launch_bounds__(256) void sources_face_lists_kernel(const long long n_tri, const int n_mesh,
                                                                 const int *__restrict__ mesh_layer,
                                                                 const long long *__restrict__ toff, const double *__restrict__ cen,
                                                                 const int n_source, const int *__restrict__ src_layer,
                                                                 const double *__restrict__ box, const int *__restrict__ poly_ptr,
                                                                 const double *__restrict__ poly_xy, const int *__restrict__ owner,
                                                                 int *__restrict__ count, const int *__restrict__ fptr,
                                                                 int *__restrict__ fsrc) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int layer = mesh_layer[find_segment(toff, n_mesh, t)];
    const double cx = cen[2 * t], cy = cen[2 * t + 1];
    int n = 0;
    const int at = FILL ? fptr[t] : 0;
    for (int s = 0; s < n_source; ++s) {
        if (src_layer[s] != layer) continue;
        const int o = owner[s];
        const bool hit = o >= 0 ? (long long)o == t
                                : source_covers(box + 4 * s, poly_xy + 2 * (long long)poly_ptr[s], poly_ptr[s + 1] - poly_ptr[s], cx, cy);
        if (hit) {
            if (FILL) fsrc[at + n] = s;
            ++n;
        }
    }
    if (!FILL) count[t] = n;
}

// b[q][v] += the load of vertex v stated at the top, for the nq <= kThermalChunk columns that start at power and b.  One
// thread per vertex, one walk of its lists for all columns
__global__ __launch_bounds__(256) void sources_load_kernel(const long long n_vert, const long long n_pot, const int *__restrict__ vptr,
                                                           const int *__restrict__ vface, const double *__restrict__ area,
                                                           const int *__restrict__ fptr, const int *__restrict__ fsrc,
                                                           const double *__restrict__ A, const int n_source, const int nq,
                                                           const double *__restrict__ power, double *__restrict__ b) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    double acc[kThermalChunk];
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q) acc[q] = 0.0;
    for (int e = vptr[v], e1 = vptr[v + 1]; e < e1; ++e) {
        const long long f = vface[e];
        const int k1 = fptr[f + 1];
        if (fptr[f] == k1) continue;
        const double af = area[f];
        for (int k = fptr[f]; k < k1; ++k) {
            const int s = fsrc[k];
            const double wgt = af / A[s];
#pragma unroll
            for (int q = 0; q < kThermalChunk; ++q)
                if (q < nq) acc[q] = acc[q] + (wgt * power[(long long)q * n_source + s]) / 3;
        }
    }
#pragma unroll
    for (int q = 0; q < kThermalChunk; ++q)
        if (q < nq) b[(long long)q * n_pot + v] = b[(long long)q * n_pot + v] + acc[q];
}

template <typename T> static int sources_keep(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

template <typename T> static int sources_upload(padne_ctx *ctx, Scratch &sc, T **out, const std::vector<T> &host) {
    PADNE_TRY(sc.alloc(out, host.size()));
    if (!host.empty())
        PADNE_HIP_CHECK(hipMemcpyAsync(*out, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, ctx->stream));
    return PADNE_OK;
}

// thermal_form_load's hook: the load of the handle's sources added to b[n_cols][n_pot] on the device, after the face gather
// and the node-heat triples.  A handle with sources forms no load without powers for exactly n_cols columns
int sources_add_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *d_b) {
    const padne_sources *sr = th->sources;
    if (sr == nullptr) return PADNE_OK;
    PADNE_REQUIRE(sr->power != nullptr && sr->power_cols == n_cols,
                  "the handle has heat sources: padne_thermal_source_power must give their powers for as many columns as the load has");
    if (th->n_vert == 0) return PADNE_OK;
    for (int c0 = 0; c0 < n_cols; c0 += kThermalChunk) {
        const int nq = n_cols - c0 < kThermalChunk ? n_cols - c0 : kThermalChunk;
        hipLaunchKernelGGL(sources_load_kernel, dim3(nblk(th->n_vert)), dim3(256), 0, ctx->stream, th->n_vert, th->n_pot,
                           (const int *)th->vptr, (const int *)th->vface, (const double *)sr->face_area, (const int *)sr->fptr,
                           (const int *)sr->fsrc, (const double *)sr->A, sr->n_source, nq,
                           (const double *)(sr->power + (size_t)c0 * (size_t)sr->n_source), d_b + (size_t)c0 * (size_t)th->n_pot);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    return PADNE_OK;
}

// the lists, A_s and the face -> sources lists of `sr` on the device; counts_out, fallback_out and area_out as the entry
// states them
static int sources_build(padne_ctx *ctx, const padne_thermal *th, padne_sources *sr, const std::vector<int> &mesh_layer,
                         const std::vector<int> &poly_ptr, const std::vector<double> &poly_xy, int64_t *counts_out,
                         int32_t *fallback_out, double *area_out) {
    hipStream_t s = ctx->stream;
    const ErrorMesh M = error_mesh_of(th->L);
    const int n_mesh = th->n_mesh, ns = sr->n_source;
    const long long n_tri = th->n_tri;
    // per source: the box (widened in x: see the top) and the vertex mean
    std::vector<double> box(4 * (size_t)ns), q(2 * (size_t)ns);
    for (int i = 0; i < ns; ++i) {
        double xlo = INFINITY, ylo = INFINITY, xhi = -INFINITY, yhi = -INFINITY, sx = 0.0, sy = 0.0;
        const int n = poly_ptr[(size_t)i + 1] - poly_ptr[(size_t)i];
        for (int k = poly_ptr[(size_t)i]; k < poly_ptr[(size_t)i + 1]; ++k) {
            const double x = poly_xy[2 * (size_t)k], y = poly_xy[2 * (size_t)k + 1];
            xlo = std::fmin(xlo, x);
            xhi = std::fmax(xhi, x);
            ylo = std::fmin(ylo, y);
            yhi = std::fmax(yhi, y);
            sx = sx + x;
            sy = sy + y;
        }
        const double margin = 1e-9 * ((xhi - xlo) + std::fmax(std::fabs(xlo), std::fabs(xhi)));
        box[4 * (size_t)i] = xlo - margin;
        box[4 * (size_t)i + 1] = ylo;
        box[4 * (size_t)i + 2] = xhi + margin;
        box[4 * (size_t)i + 3] = yhi;
        q[2 * (size_t)i] = sx / n;
        q[2 * (size_t)i + 1] = sy / n;
    }
    Scratch sc(ctx);
    int *d_mesh_layer = nullptr, *d_src_layer = nullptr, *d_poly_ptr = nullptr, *d_count = nullptr, *d_owner = nullptr, *d_bad = nullptr;
    double *d_box = nullptr, *d_q = nullptr, *d_poly = nullptr, *d_cen = nullptr;
    PADNE_TRY(sources_upload(ctx, sc, &d_mesh_layer, mesh_layer));
    PADNE_TRY(sources_upload(ctx, sc, &d_src_layer, sr->layer));
    PADNE_TRY(sources_upload(ctx, sc, &d_poly_ptr, poly_ptr));
    PADNE_TRY(sources_upload(ctx, sc, &d_box, box));
    PADNE_TRY(sources_upload(ctx, sc, &d_q, q));
    PADNE_TRY(sources_upload(ctx, sc, &d_poly, poly_xy));
    PADNE_TRY(sc.alloc(&d_count, (size_t)ns));
    PADNE_TRY(sc.alloc(&d_owner, (size_t)ns));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_TRY(sc.alloc(&d_cen, 2 * (size_t)n_tri));
    PADNE_TRY(sources_keep(ctx, &sr->face_area, (size_t)n_tri));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (n_tri > 0) {
        hipLaunchKernelGGL(sources_face_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, n_tri, n_mesh, M.tri, M.xy, M.voff, M.toff,
                           sr->face_area, d_cen, d_bad);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    // the count pass, then the owners of the sources that cover nothing
    hipLaunchKernelGGL(sources_walk_kernel<false>, dim3((unsigned)ns), dim3(256), 0, s, n_mesh, (const int *)d_mesh_layer, M.toff,
                       (const double *)d_cen, (const int *)d_src_layer, (const double *)d_box, (const int *)d_poly_ptr,
                       (const double *)d_poly, (const int *)nullptr, (const int *)nullptr, (int *)nullptr, d_count);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<int> count((size_t)ns), owner((size_t)ns, -1);
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(count.data(), d_count, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    PADNE_REQUIRE(!h_bad, "triangle index out of range");
    bool some_empty = false;
    for (int i = 0; i < ns; ++i) some_empty = some_empty || count[(size_t)i] == 0;
    if (some_empty) {
        hipLaunchKernelGGL(sources_owner_kernel, dim3((unsigned)ns), dim3(256), 0, s, n_mesh, (const int *)d_mesh_layer, M.toff, M.voff,
                           M.tri, M.xy, (const int *)d_src_layer, (const int *)d_count, (const double *)d_q, d_owner);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(owner.data(), d_owner, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        PADNE_HIP_CHECK(hipMemsetAsync(d_owner, 0xff, sizeof(int) * (size_t)ns, s));      // -1: no fallback
    }
    sr->lptr_host.assign((size_t)ns + 1, 0);
    int off_copper = -1;
    for (int i = 0; i < ns; ++i) {
        const bool fallback = count[(size_t)i] == 0;
        const bool lost = fallback && owner[(size_t)i] == kNoOwner;
        if (lost && off_copper < 0) off_copper = i;
        counts_out[i] = lost ? 0 : (fallback ? 1 : count[(size_t)i]);
        fallback_out[i] = lost ? 2 : (fallback ? 1 : 0);
        sr->lptr_host[(size_t)i + 1] = sr->lptr_host[(size_t)i] + counts_out[i];
    }
    if (off_copper >= 0) {
        set_error("invalid argument: heat source %d lies on no copper of layer %d that the system keeps", off_copper,
                  sr->layer[(size_t)off_copper]);
        return PADNE_E_INVALID;
    }
    sr->n_entries = sr->lptr_host[(size_t)ns];
    PADNE_REQUIRE(sr->n_entries <= 0x7fffffffLL, "too many (source, face) pairs for 32-bit lists");
    std::vector<int> lptr(sr->lptr_host.begin(), sr->lptr_host.end());
    PADNE_TRY(sources_keep(ctx, &sr->lptr, (size_t)ns + 1));
    PADNE_TRY(sources_keep(ctx, &sr->lface, (size_t)sr->n_entries));
    PADNE_TRY(sources_keep(ctx, &sr->A, (size_t)ns));
    PADNE_HIP_CHECK(hipMemcpyAsync(sr->lptr, lptr.data(), sizeof(int) * ((size_t)ns + 1), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sources_walk_kernel<true>, dim3((unsigned)ns), dim3(256), 0, s, n_mesh, (const int *)d_mesh_layer, M.toff,
                       (const double *)d_cen, (const int *)d_src_layer, (const double *)d_box, (const int *)d_poly_ptr,
                       (const double *)d_poly, (const int *)d_owner, (const int *)sr->lptr, sr->lface, (int *)nullptr);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sources_sum_kernel<false>, dim3((unsigned)ns), dim3(256), 0, s, ns, (const int *)sr->lptr, (const int *)sr->lface,
                       (const double *)sr->face_area, (const double *)nullptr, n_mesh, M.tri, M.voff, M.toff, th->n_pot,
                       (const double *)nullptr, sr->A);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(area_out, sr->A, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
    // face -> sources: count, scan, fill
    int *d_fcount = nullptr;
    PADNE_TRY(sc.alloc(&d_fcount, (size_t)n_tri));
    PADNE_TRY(sources_keep(ctx, &sr->fptr, (size_t)n_tri + 1));
    if (n_tri > 0) {
        hipLaunchKernelGGL(sources_face_lists_kernel<false>, dim3(nblk(n_tri)), dim3(256), 0, s, n_tri, n_mesh, (const int *)d_mesh_layer,
                           M.toff, (const double *)d_cen, ns, (const int *)d_src_layer, (const double *)d_box, (const int *)d_poly_ptr,
                           (const double *)d_poly, (const int *)d_owner, d_fcount, (const int *)nullptr, (int *)nullptr);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    int64_t total = 0;
    PADNE_TRY(exclusive_scan_i32(ctx, d_fcount, sr->fptr, n_tri, &total));
    PADNE_REQUIRE(total == sr->n_entries, "the face lists and the source lists disagree");
    PADNE_TRY(sources_keep(ctx, &sr->fsrc, (size_t)total));
    if (n_tri > 0) {
        hipLaunchKernelGGL(sources_face_lists_kernel<true>, dim3(nblk(n_tri)), dim3(256), 0, s, n_tri, n_mesh, (const int *)d_mesh_layer,
                           M.toff, (const double *)d_cen, ns, (const int *)d_src_layer, (const double *)d_box, (const int *)d_poly_ptr,
                           (const double *)d_poly, (const int *)d_owner, (int *)nullptr, (const int *)sr->fptr, sr->fsrc);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));               // (the uploads read the host vectors above before they go)
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_thermal_set_sources(padne_ctx *ctx, padne_thermal *th, int32_t n_layer, int32_t n_mesh, const int32_t *mesh_layer,
                                         int32_t n_source, const int32_t *source_layer, const int64_t *poly_ptr, const double *poly_xy,
                                         int64_t *counts_out, int32_t *fallback_out, double *area_out) {
    PADNE_TRY(thermal_require("padne_thermal_set_sources", ctx, th));
    PADNE_REQUIRE(n_layer >= 1 && n_source >= 0 && n_source <= kSourceMaxCount, "at least one layer, between 0 and 4096 heat sources");
    PADNE_REQUIRE(n_mesh == th->n_mesh, "n_mesh must be that of the system's mesh");
    PADNE_REQUIRE(n_source == 0 || th->n_tri > 0, "heat sources need a mesh with faces");
    PADNE_REQUIRE(mesh_layer != nullptr || n_mesh == 0, "null argument");
    PADNE_REQUIRE(n_source == 0 || (source_layer && poly_ptr && poly_xy && counts_out && fallback_out && area_out), "null argument");
    for (int32_t m = 0; m < n_mesh; ++m) PADNE_REQUIRE(mesh_layer[m] >= 0 && mesh_layer[m] < n_layer, "mesh layer out of range");
    PADNE_REQUIRE(n_source == 0 || poly_ptr[0] == 0, "poly_ptr starts at 0");
    for (int32_t i = 0; i < n_source; ++i) {
        PADNE_REQUIRE(source_layer[i] >= 0 && source_layer[i] < n_layer, "source layer out of range");
        PADNE_REQUIRE(poly_ptr[i + 1] >= poly_ptr[i] + 3 && poly_ptr[i + 1] - poly_ptr[i] <= kSourceMaxVertices,
                      "poly_ptr ascends by 3 to 256 vertices per polygon");
    }
    for (int64_t k = 0; n_source > 0 && k < 2 * poly_ptr[n_source]; ++k)
        PADNE_REQUIRE(std::isfinite(poly_xy[k]), "polygon coordinates must be finite");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    sources_free(ctx, th->sources);                          // a second call replaces the first
    th->sources = nullptr;
    if (n_source == 0) return PADNE_OK;
    padne_sources *sr = new padne_sources;
    sr->n_source = n_source;
    sr->n_layer = n_layer;
    sr->layer.assign(source_layer, source_layer + n_source);
    const std::vector<int> ml(mesh_layer, mesh_layer + n_mesh), pp(poly_ptr, poly_ptr + n_source + 1);
    const std::vector<double> pxy(poly_xy, poly_xy + 2 * poly_ptr[n_source]);
    const int rc = sources_build(ctx, th, sr, ml, pp, pxy, counts_out, fallback_out, area_out);
    if (rc != PADNE_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        sources_free(ctx, sr);
        return rc;
    }
    th->sources = sr;
    return PADNE_OK;
}

extern "C" int padne_thermal_source_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *power) {
    PADNE_TRY(thermal_require("padne_thermal_source_power", ctx, th));
    PADNE_REQUIRE(th->sources != nullptr, "padne_thermal_source_power follows padne_thermal_set_sources");
    PADNE_REQUIRE(n_cols >= 1 && n_cols <= 4096 && power != nullptr, "between 1 and 4096 columns of powers");
    padne_sources *sr = th->sources;
    const size_t count = (size_t)n_cols * (size_t)sr->n_source;
    for (size_t i = 0; i < count; ++i) PADNE_REQUIRE(std::isfinite(power[i]) && power[i] >= 0.0, "a power must be finite and not negative");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    if (sr->power != nullptr) pool_free(ctx, sr->power);
    sr->power_cols = 0;
    sr->power = (double *)pool_alloc(ctx, sizeof(double) * count);
    if (sr->power == nullptr) return PADNE_E_NOMEM;
    PADNE_HIP_CHECK(hipMemcpyAsync(sr->power, power, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    sr->power_cols = n_cols;
    return PADNE_OK;
}

extern "C" int padne_thermal_source_lists(padne_ctx *ctx, const padne_thermal *th, int32_t n_source, int64_t n_entries, int64_t *ptr_out,
                                          int32_t *face_out) {
    PADNE_TRY(thermal_require("padne_thermal_source_lists", ctx, th));
    PADNE_REQUIRE(th->sources != nullptr, "padne_thermal_source_lists follows padne_thermal_set_sources");
    const padne_sources *sr = th->sources;
    PADNE_REQUIRE(n_source == sr->n_source && n_entries == sr->n_entries, "n_source and n_entries must be those of padne_thermal_set_sources");
    PADNE_REQUIRE(ptr_out && (n_entries == 0 || face_out), "null argument");
    for (size_t i = 0; i < sr->lptr_host.size(); ++i) ptr_out[i] = sr->lptr_host[i];
    if (n_entries == 0) return PADNE_OK;
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    PADNE_HIP_CHECK(hipMemcpyAsync(face_out, sr->lface, sizeof(int) * (size_t)n_entries, hipMemcpyDeviceToHost, ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PADNE_OK;
}

// out_host[n_cols][n_source] = the sum over every source's list, in the order of A_s, of (area_f / A_s) * the face mean of the
// field[n_cols][n_pot] on the device: the report of theta, and of an adjoint field for thermal_sens.hip
int padne::sources_report_field(padne_ctx *ctx, const padne_thermal *th, int32_t n_cols, const double *field, double *out_host) {
    PADNE_REQUIRE(n_cols >= 1 && n_cols <= 65535, "too many columns for one launch");
    PADNE_REQUIRE(out_host != nullptr, "null argument");
    const padne_sources *sr = th->sources;
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const ErrorMesh M = error_mesh_of(th->L);
    const size_t count = (size_t)n_cols * (size_t)sr->n_source;
    Scratch sc(ctx);
    double *d_out = nullptr;
    PADNE_TRY(sc.alloc(&d_out, count));
    hipLaunchKernelGGL(sources_sum_kernel<true>, dim3((unsigned)sr->n_source, (unsigned)n_cols), dim3(256), 0, s, sr->n_source,
                       (const int *)sr->lptr, (const int *)sr->lface, (const double *)sr->face_area, (const double *)sr->A, th->n_mesh,
                       M.tri, M.voff, M.toff, th->n_pot, field, d_out);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_thermal_source_report(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *temperature_out) {
    PADNE_TRY(thermal_require("padne_thermal_source_report", ctx, th));
    PADNE_REQUIRE(th->sources != nullptr, "padne_thermal_source_report follows padne_thermal_set_sources");
    PADNE_REQUIRE(th->solved && n_cols == th->n_cols, "padne_thermal_source_report follows a solve of as many columns");
    return sources_report_field(ctx, th, n_cols, th->theta, temperature_out);
}
