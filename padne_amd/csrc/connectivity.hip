// The connectivity pre-pass ("Connectivity pre-pass"): which polygons of a board does every connection point touch.
// Stands where the reference's STRtree query and shapely's intersects / contains stand (padne/solver.py:84-148, 263-330); the
// graph over the answers is host work (padne_amd/solver.py, compute_connectivity).  One call locates a batch of query points
// in a batch of polygons; tests/connectivity_ref.py restates the rule in numpy, and the two agree in every bit.
//
//   polygons  as padne_polymesh_create takes them: polygon p = the rings poly_ring_ptr[p] .. poly_ring_ptr[p + 1] (exterior,
//             holes; orientation free), ring r = the n >= 3 vertices ring_ptr[r] .. ring_ptr[r + 1] of ring_xy, without a
//             closing duplicate;
//   groups    polygon p belongs to group poly_group[p] >= 0 (its layer), ascending over the batch; query q to
//             query_group[q] >= 0.  A query meets the polygons of its own group only; a group without polygons is valid;
//   segments  for every ring vertex i the segment from the previous vertex of the same ring (cyclic) (xj, yj) to (xi, yi);
//   box       of a polygon: the exact least and greatest x and y of its ring vertices.  A query outside the closed box
//             (px < xmin, px > xmax, py < ymin or py > ymax) has kind 0 and the segments are not read;
//   crossing  a segment crosses when (yi > py) != (yj > py) && px < (xj - xi) * (py - yi) / (yj - yi) + xi, the rule of
//             sources.hip, rounded as written; inside when the crossings over all rings are odd;
//   boundary  on when for some segment (xi - xj) * (py - yj) - (yi - yj) * (px - xj) == 0 and
//             min(xi, xj) <= px <= max(xi, xj) and min(yi, yj) <= py <= max(yi, yj);
//   kind      of (query, polygon): 2 when on, else 1 when inside, else 0.  A hit is kind != 0 (shapely's intersects for a
//             point), kind 1 is contains;
//   output    CSR over the queries: hit_ptr[n_query + 1], and per hit the polygon and the kind, a query's hits in ascending
//             polygon number.
//
// The boundary test is exact and carries no tolerance: it sees every ring vertex, every point of an axis-parallel segment and
// every point where the two products are exact.  A point computed onto a slanted segment is in general not seen as on it and
// then counts by parity, on either side.  The reference's predicate is as strict.
//
// The box: an on point lies in its segment's box, an inside point has a segment that straddles py, so the y limits follow
// from comparisons alone.  The x limits hold up to the rounding of the crossing abscissa; so that no rounding can make the
// answer depend on whether the box was asked, the box is part of the rule and the restatement tests it too.
//
// Kernels.  polygons_segment_kernel: one thread per ring vertex writes its segment (xj, yj, xi, yi), 32 B.
// polygons_box_kernel: a wave per polygon, min / max over its vertices by xor shuffles (exact, order free).
// polygons_locate_kernel<FILL>: a wave per query, four queries per workgroup of 256.  The wave runs over the polygons of the
// query's group 64 at a time, one closed box test per lane; the 64-bit ballot hands out the candidates in ascending order;
// for each candidate the lanes stride over its segments, every lane keeps a crossing parity and an on bit, joined by
// popcount(ballot) and ballot != 0.  Parity and the on bit are integers that do not depend on the order, so however the
// segments are dealt to lanes the result is the restatement's.  FILL = false counts the hits of every query, an exclusive
// scan makes hit_ptr, FILL = true writes them; both run polygons_locate_wave.  No floating-point atomics, no atomics at all.
// Compiled with -ffp-contract=off.
//
// What a call must read: 32 B of box per (query, polygon of its group) and 32 B per segment of every candidate (a polygon
// whose box holds the query), in each of the two passes; the boxes of a group are shared by all its queries and stay in L2.
// The double division sits behind the straddle test, as in source_covers.
//
// Limits: fewer than 2^31 segments and fewer than 2^31 hits (PADNE_E_TOOLARGE).  One GPU.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace padne {

// seg[4 v ..] = (xj, yj, xi, yi) for ring vertex v; the ring of v by bisection over ring_ptr
__global__ __launch_bounds__(256) void polygons_segment_kernel(const int n_vert, const int n_ring, const int *__restrict__ ring_ptr,
                                                               const double *__restrict__ ring_xy, double *__restrict__ seg) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    int lo = 0, hi = n_ring - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ring_ptr[mid] <= v) lo = mid; else hi = mid - 1;
    }
    const int prev = v == ring_ptr[lo] ? ring_ptr[lo + 1] - 1 : v - 1;
    seg[4 * (long long)v] = ring_xy[2 * (long long)prev];
    seg[4 * (long long)v + 1] = ring_xy[2 * (long long)prev + 1];
    seg[4 * (long long)v + 2] = ring_xy[2 * (long long)v];
    seg[4 * (long long)v + 3] = ring_xy[2 * (long long)v + 1];
}

// box[4 p ..] = (xmin, ymin, xmax, ymax) of polygon p.  A wave per polygon, four per workgroup
__global__ __launch_bounds__(256) void polygons_box_kernel(const int n_poly, const int *__restrict__ poly_seg_ptr,
                                                           const double *__restrict__ seg, double *__restrict__ box) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_poly) return;                                  // (the same for the whole wave)
    double xlo = INFINITY, ylo = INFINITY, xhi = -INFINITY, yhi = -INFINITY;
    for (int s = poly_seg_ptr[p] + lane; s < poly_seg_ptr[p + 1]; s += 64) {
        const double x = seg[4 * (long long)s + 2], y = seg[4 * (long long)s + 3];
        xlo = fmin(xlo, x);
        ylo = fmin(ylo, y);
        xhi = fmax(xhi, x);
        yhi = fmax(yhi, y);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        xlo = fmin(xlo, __shfl_xor(xlo, d));
        ylo = fmin(ylo, __shfl_xor(ylo, d));
        xhi = fmax(xhi, __shfl_xor(xhi, d));
        yhi = fmax(yhi, __shfl_xor(yhi, d));
    }
    if (lane == 0) {
        box[4 * (long long)p] = xlo;
        box[4 * (long long)p + 1] = ylo;
        box[4 * (long long)p + 2] = xhi;
        box[4 * (long long)p + 3] = yhi;
    }
}

// The hits of the query (px, py) among the polygons lo .. hi, by the whole wave: hit(polygon, kind) is called in ascending
// polygon order, with the same arguments in every lane.  Returns their number
template <typename Hit>
__device__ __forceinline__ int polygons_locate_wave(const int lane, const int lo, const int hi, const double px, const double py,
                                                    const double *__restrict__ box, const int *__restrict__ poly_seg_ptr,
                                                    const double *__restrict__ seg, Hit hit) {
    int n = 0;
    for (int p0 = lo; p0 < hi; p0 += 64) {
        const int p = p0 + lane;
        bool cand = false;
        if (p < hi) {
            const double *b = box + 4 * (long long)p;
            cand = px >= b[0] && px <= b[2] && py >= b[1] && py <= b[3];
        }
        unsigned long long todo = __ballot(cand);
        while (todo != 0) {                                   // (the same in every lane)
            const int c = p0 + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            bool odd = false, on = false;
            for (int s = poly_seg_ptr[c] + lane; s < poly_seg_ptr[c + 1]; s += 64) {
                const double *g = seg + 4 * (long long)s;
                const double xj = g[0], yj = g[1], xi = g[2], yi = g[3];
                if ((yi > py) != (yj > py) && px < (xj - xi) * (py - yi) / (yj - yi) + xi) odd = !odd;
                if ((xi - xj) * (py - yj) - (yi - yj) * (px - xj) == 0.0 && fmin(xi, xj) <= px && px <= fmax(xi, xj) &&
                    fmin(yi, yj) <= py && py <= fmax(yi, yj))
                    on = true;
            }
            const bool inside = (__popcll(__ballot(odd)) & 1) != 0;
            const int kind = __ballot(on) != 0 ? 2 : inside ? 1 : 0;
            if (kind != 0) {
                hit(c, kind);
                ++n;
            }
        }
    }
    return n;
}

// FILL = false: count[q] = the hits of query q.  FILL = true: they are written from hit_ptr[q] on
template <bool FILL>
__global__ __launch_bounds__(256) void polygons_locate_kernel(const int n_query, const double *__restrict__ query_xy,
                                                              const int *__restrict__ query_range, const double *__restrict__ box,
                                                              const int *__restrict__ poly_seg_ptr, const double *__restrict__ seg,
                                                              int *__restrict__ count, const int *__restrict__ hit_ptr,
                                                              int *__restrict__ hit_poly, int *__restrict__ hit_kind) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= n_query) return;                                 // (the same for the whole wave)
    const double px = query_xy[2 * (long long)q], py = query_xy[2 * (long long)q + 1];
    const int lo = query_range[2 * (long long)q], hi = query_range[2 * (long long)q + 1];
    if (FILL) {
        int at = hit_ptr[q];
        polygons_locate_wave(lane, lo, hi, px, py, box, poly_seg_ptr, seg, [&](int c, int kind) {
            if (lane == 0) {
                hit_poly[at] = c;
                hit_kind[at] = kind;
            }
            ++at;
        });
    } else {
        const int n = polygons_locate_wave(lane, lo, hi, px, py, box, poly_seg_ptr, seg, [](int, int) {});
        if (lane == 0) count[q] = n;
    }
}

}  // namespace padne

using namespace padne;

struct padne_polyhits {
    padne_ctx *owner = nullptr;
    int64_t n_query = 0, n_hit = 0;
    // device (the owner's pool); hit_ptr == nullptr: no hit at all, every offset is 0
    int *hit_ptr = nullptr, *hit_poly = nullptr, *hit_kind = nullptr;
};

static void polyhits_free(padne_polyhits *ph) {
    if (ph == nullptr) return;
    void *blocks[] = {ph->hit_ptr, ph->hit_poly, ph->hit_kind};
    for (void *p : blocks)
        if (p) pool_free(ph->owner, p);
    delete ph;
}

template <typename T> static int polyhits_alloc(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

extern "C" int padne_polygons_locate(padne_ctx *ctx, int64_t n_poly, const int64_t *poly_ring_ptr, const int64_t *ring_ptr,
                                     const double *ring_xy, const int32_t *poly_group, int64_t n_query, const double *query_xy,
                                     const int32_t *query_group, int64_t *hit_count_out, padne_polyhits **out) {
    PADNE_REQUIRE(ctx && out && hit_count_out, "null argument");
    *out = nullptr;
    *hit_count_out = 0;
    PADNE_REQUIRE(n_poly >= 0 && n_query >= 0, "negative count");
    PADNE_REQUIRE(n_poly == 0 || (poly_ring_ptr && ring_ptr && ring_xy && poly_group), "null argument");
    PADNE_REQUIRE(n_query == 0 || (query_xy && query_group), "null argument");
    if (n_poly >= 0x7fffffffLL / 3 || n_query >= 0x7fffffffLL - 256) {
        set_error("%lld polygons and %lld queries exceed the 32-bit index space", (long long)n_poly, (long long)n_query);
        return PADNE_E_TOOLARGE;
    }
    // ---- the checks, the segment offsets of the polygons and the polygon range of every query, on the host
    std::vector<int> ring_ptr32, poly_seg_ptr((size_t)n_poly + 1, 0), query_range(2 * (size_t)n_query, 0);
    int64_t n_ring = 0, n_vert = 0;
    if (n_poly > 0) {
        PADNE_REQUIRE(poly_ring_ptr[0] == 0 && ring_ptr[0] == 0, "offset tables must start at 0");
        for (int64_t p = 0; p < n_poly; ++p) {
            PADNE_REQUIRE(poly_ring_ptr[p + 1] > poly_ring_ptr[p], "a polygon has at least its exterior ring");
            PADNE_REQUIRE(poly_group[p] >= 0, "a group is not negative");
            PADNE_REQUIRE(p == 0 || poly_group[p] >= poly_group[p - 1], "the groups of the polygons must be ascending");
        }
        n_ring = poly_ring_ptr[n_poly];
        ring_ptr32.resize((size_t)n_ring + 1);
        ring_ptr32[0] = 0;
        for (int64_t r = 0; r < n_ring; ++r) {
            PADNE_REQUIRE(ring_ptr[r + 1] - ring_ptr[r] >= 3, "a ring has at least 3 vertices");
            if (ring_ptr[r + 1] >= 0x7fffffffLL) {
                set_error("2^31 segments or more exceed the 32-bit index space");
                return PADNE_E_TOOLARGE;
            }
            ring_ptr32[(size_t)r + 1] = (int)ring_ptr[r + 1];
        }
        n_vert = ring_ptr[n_ring];
        for (int64_t k = 0; k < 2 * n_vert; ++k) PADNE_REQUIRE(std::isfinite(ring_xy[k]), "a coordinate is not finite");
        for (int64_t p = 0; p <= n_poly; ++p) poly_seg_ptr[(size_t)p] = ring_ptr32[(size_t)poly_ring_ptr[p]];
    }
    for (int64_t q = 0; q < n_query; ++q) {
        PADNE_REQUIRE(std::isfinite(query_xy[2 * q]) && std::isfinite(query_xy[2 * q + 1]), "a query point is not finite");
        PADNE_REQUIRE(query_group[q] >= 0, "a group is not negative");
        if (n_poly > 0) {
            const int32_t *lo = std::lower_bound(poly_group, poly_group + n_poly, query_group[q]);
            const int32_t *hi = std::upper_bound(lo, poly_group + n_poly, query_group[q]);
            query_range[2 * (size_t)q] = (int)(lo - poly_group);
            query_range[2 * (size_t)q + 1] = (int)(hi - poly_group);
        }
    }
    padne_polyhits *ph = new padne_polyhits;
    ph->owner = ctx;
    ph->n_query = n_query;
    if (n_poly == 0 || n_query == 0) {                        // an empty result, without a launch
        *out = ph;
        return PADNE_OK;
    }
    struct Guard {      // an error path hands everything back
        padne_polyhits *ph;
        ~Guard() { polyhits_free(ph); }
    } guard{ph};
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int np = (int)n_poly, nq = (int)n_query, nv = (int)n_vert, nr = (int)n_ring;
    Scratch sc(ctx);
    int *d_ring_ptr = nullptr, *d_poly_seg_ptr = nullptr, *d_range = nullptr, *d_count = nullptr;
    double *d_ring_xy = nullptr, *d_seg = nullptr, *d_box = nullptr, *d_query = nullptr;
    PADNE_TRY(sc.alloc(&d_ring_ptr, (size_t)nr + 1));
    PADNE_TRY(sc.alloc(&d_poly_seg_ptr, (size_t)np + 1));
    PADNE_TRY(sc.alloc(&d_range, 2 * (size_t)nq));
    PADNE_TRY(sc.alloc(&d_count, (size_t)nq));
    PADNE_TRY(sc.alloc(&d_ring_xy, 2 * (size_t)nv));
    PADNE_TRY(sc.alloc(&d_seg, 4 * (size_t)nv));
    PADNE_TRY(sc.alloc(&d_box, 4 * (size_t)np));
    PADNE_TRY(sc.alloc(&d_query, 2 * (size_t)nq));
    PADNE_TRY(polyhits_alloc(ctx, &ph->hit_ptr, (size_t)nq + 1));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ring_ptr, ring_ptr32.data(), sizeof(int) * ((size_t)nr + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_poly_seg_ptr, poly_seg_ptr.data(), sizeof(int) * ((size_t)np + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_range, query_range.data(), sizeof(int) * 2 * (size_t)nq, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ring_xy, ring_xy, sizeof(double) * 2 * (size_t)nv, hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_query, query_xy, sizeof(double) * 2 * (size_t)nq, hipMemcpyHostToDevice, s));

    hipLaunchKernelGGL(polygons_segment_kernel, dim3(nblk(nv)), dim3(256), 0, s, nv, nr, (const int *)d_ring_ptr,
                       (const double *)d_ring_xy, d_seg);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(polygons_box_kernel, dim3(nblk(np, 4)), dim3(256), 0, s, np, (const int *)d_poly_seg_ptr, (const double *)d_seg,
                       d_box);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(polygons_locate_kernel<false>, dim3(nblk(nq, 4)), dim3(256), 0, s, nq, (const double *)d_query,
                       (const int *)d_range, (const double *)d_box, (const int *)d_poly_seg_ptr, (const double *)d_seg, d_count,
                       (const int *)nullptr, (int *)nullptr, (int *)nullptr);
    PADNE_HIP_CHECK(hipGetLastError());
    int64_t n_hit = 0;
    PADNE_TRY(exclusive_scan_i32(ctx, d_count, ph->hit_ptr, nq, &n_hit));
    ph->n_hit = n_hit;
    PADNE_TRY(polyhits_alloc(ctx, &ph->hit_poly, (size_t)n_hit));
    PADNE_TRY(polyhits_alloc(ctx, &ph->hit_kind, (size_t)n_hit));
    if (n_hit > 0) {
        hipLaunchKernelGGL(polygons_locate_kernel<true>, dim3(nblk(nq, 4)), dim3(256), 0, s, nq, (const double *)d_query,
                           (const int *)d_range, (const double *)d_box, (const int *)d_poly_seg_ptr, (const double *)d_seg,
                           (int *)nullptr, (const int *)ph->hit_ptr, ph->hit_poly, ph->hit_kind);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    *hit_count_out = n_hit;
    guard.ph = nullptr;
    *out = ph;
    return PADNE_OK;
}

extern "C" int padne_polygons_locate_fetch(padne_ctx *ctx, const padne_polyhits *ph, int32_t *hit_ptr_out, int32_t *hit_poly_out,
                                           int32_t *hit_kind_out) {
    PADNE_REQUIRE(ctx && ph && hit_ptr_out, "null argument");
    PADNE_REQUIRE(ctx == ph->owner, "a batch of hits is fetched through the context that made it");
    PADNE_REQUIRE(ph->n_hit == 0 || (hit_poly_out && hit_kind_out), "null argument");
    if (ph->hit_ptr == nullptr) {
        for (int64_t q = 0; q <= ph->n_query; ++q) hit_ptr_out[q] = 0;
        return PADNE_OK;
    }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PADNE_HIP_CHECK(hipMemcpyAsync(hit_ptr_out, ph->hit_ptr, sizeof(int32_t) * ((size_t)ph->n_query + 1), hipMemcpyDeviceToHost, s));
    if (ph->n_hit > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(hit_poly_out, ph->hit_poly, sizeof(int32_t) * (size_t)ph->n_hit, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(hit_kind_out, ph->hit_kind, sizeof(int32_t) * (size_t)ph->n_hit, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_polygons_locate_destroy(padne_polyhits *ph) {
    if (ph == nullptr) return PADNE_OK;
    if (ph->owner) {
        (void)hipSetDevice(ph->owner->device);
        (void)hipStreamSynchronize(ph->owner->stream);
    }
    polyhits_free(ph);
    return PADNE_OK;
}
