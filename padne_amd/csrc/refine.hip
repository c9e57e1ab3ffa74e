// Mesh refinement where an error estimate asks for it ("Refinement"): 4-triangle longest-edge refinement with
// conforming closure, on the two flat arrays of a batch of meshes.  No reference counterpart.  The first kernels of the
// library that produce topology; the idiom is error.hip's: sort keys, scan, emit, no atomics, two calls give the same bits.
//   edges     corner c of face f runs (tri[f][c], tri[f][(c + 1) % 3]); key = lo * n_vert + hi over global vertex numbers;
//             the edges are the distinct keys in ascending order: (key, slot) per corner, one stable radix sort, run heads,
//             an exclusive scan, the edge number scattered back to every corner.  A run longer than two, or two corners
//             that run an edge in the same direction, is a non-manifold mesh;
//   lengths   d_e = dx * dx + dy * dy from lo to hi (one value per edge, so its two faces see the same bits); the longest
//             edge of a face is the one with the greatest d_e, the lowest edge number on a tie;
//   marks     every edge of a flagged face, then the closure: while a face has a marked edge and its longest unmarked, mark
//             the longest.  Marks only grow and the rule is monotone: the result is the least fixed point whatever the order
//             of the stores, which are plain idempotent stores of 1 into a 32-bit word per edge;
//   emit      one new vertex per marked edge behind the old vertices of its mesh in ascending edge number, 1 + (marked edges)
//             children per face in parent order: a scan of the marks, a scan of the child counts, one kernel each.
// Everything is bound by memory; refine_emit_kernel holds a face's twelve indices in registers and spills nothing.
#include "common.hpp"
#include "face.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <vector>

namespace padne {

constexpr int kSweepsPerLook = 4;      // closure sweeps queued between two looks at the "changed" word

enum { REFINE_BAD_INDEX = 0, REFINE_REPEATED = 1, REFINE_NONMANIFOLD = 2, REFINE_ERR_WORDS = 4 };

// key[3 t + c] = lo * n_vert + hi of corner c of face t, val = (3 t + c) << 1 | (the corner runs from lo to hi).  A face
// with an index out of range or a vertex named twice is reported and given distinct harmless keys (nothing after the sort
// reads a vertex before the report has been looked at).
template <typename Key>
__global__ __launch_bounds__(256) void refine_corner_kernel(const long long n_tri, const long long n_vert, const int n_mesh,
                                                            const int32_t *__restrict__ tri, const long long *__restrict__ voff,
                                                            const long long *__restrict__ toff, Key *__restrict__ key,
                                                            unsigned *__restrict__ val, int *__restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int m = find_segment(toff, n_mesh, t);
    const long long v0 = voff[m], nv = voff[m + 1] - v0;
    long long g[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        const int l = tri[3 * t + c];
        ok = ok && l >= 0 && l < nv;
        g[c] = v0 + l;
    }
    if (!ok) *(volatile int *)(err + REFINE_BAD_INDEX) = 1;
    else if (g[0] == g[1] || g[1] == g[2] || g[2] == g[0]) {
        *(volatile int *)(err + REFINE_REPEATED) = 1;
        ok = false;
    }
    for (int c = 0; c < 3; ++c) {
        const long long u = g[c], v = g[(c + 1) % 3];
        const long long lo = u < v ? u : v, hi = u < v ? v : u;
        key[3 * t + c] = ok ? (Key)((unsigned long long)lo * (unsigned long long)n_vert + (unsigned long long)hi) : (Key)0;
        val[3 * t + c] = ((unsigned)(3 * t + c) << 1) | (u < v ? 1u : 0u);
    }
}

// head[i] = 1 where a run of equal sorted keys starts; the run-length check is the manifold test
template <typename Key>
__global__ __launch_bounds__(256) void refine_head_kernel(const long long n, const Key *__restrict__ key,
                                                          const unsigned *__restrict__ val, int *__restrict__ head,
                                                          int *__restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool first = i == 0 || key[i] != key[i - 1];
    head[i] = first ? 1 : 0;
    if (!first) {
        const bool third = i >= 2 && key[i] == key[i - 2];
        if (third || ((val[i] ^ val[i - 1]) & 1u) == 0) *(volatile int *)(err + REFINE_NONMANIFOLD) = 1;
    }
}

// the edge number of every sorted corner goes back to its slot; the head of a run writes the edge's ends and d_e
template <typename Key>
__global__ __launch_bounds__(256) void refine_edge_kernel(const long long n, const long long n_vert, const Key *__restrict__ key,
                                                          const unsigned *__restrict__ val, const int *__restrict__ head,
                                                          const int *__restrict__ before, const double *__restrict__ xy,
                                                          int *__restrict__ corner_edge, int *__restrict__ edge_lo,
                                                          int *__restrict__ edge_hi, double *__restrict__ edge_d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int h = head[i];
    const int e = before[i] + h - 1;
    corner_edge[val[i] >> 1] = e;
    if (h) {
        const unsigned long long k = (unsigned long long)key[i];
        const long long lo = (long long)(k / (unsigned long long)n_vert), hi = (long long)(k % (unsigned long long)n_vert);
        const double dx = xy[2 * hi] - xy[2 * lo], dy = xy[2 * hi + 1] - xy[2 * lo + 1];
        edge_lo[e] = (int)lo;
        edge_hi[e] = (int)hi;
        edge_d[e] = dx * dx + dy * dy;
    }
}

// longest[t] = the corner of the face's longest edge; a flagged face marks its three edges
__global__ __launch_bounds__(256) void refine_face_kernel(const long long n_tri, const int *__restrict__ corner_edge,
                                                          const double *__restrict__ edge_d, const unsigned char *__restrict__ flag,
                                                          unsigned char *__restrict__ longest, int *__restrict__ mark) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int e0 = corner_edge[3 * t], e1 = corner_edge[3 * t + 1], e2 = corner_edge[3 * t + 2];
    const double d0 = edge_d[e0], d1 = edge_d[e1], d2 = edge_d[e2];
    int best = 0, eb = e0;
    double db = d0;
    if (d1 > db || (d1 == db && e1 < eb)) {
        best = 1;
        eb = e1;
        db = d1;
    }
    if (d2 > db || (d2 == db && e2 < eb)) best = 2;
    longest[t] = (unsigned char)best;
    if (flag[t]) mark[e0] = mark[e1] = mark[e2] = 1;
}

// one closure sweep: a face with a marked edge and its longest unmarked marks the longest.  The marks are read while other
// faces store into them: a face may or may not see a mark of this sweep, and either way the fixed point is the same.
__global__ __launch_bounds__(256) void refine_sweep_kernel(const long long n_tri, const int *__restrict__ corner_edge,
                                                           const unsigned char *__restrict__ longest, int *mark, int *changed) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int e0 = corner_edge[3 * t], e1 = corner_edge[3 * t + 1], e2 = corner_edge[3 * t + 2];
    const int l = longest[t];
    const int el = l == 0 ? e0 : l == 1 ? e1 : e2;
    const volatile int *mk = mark;
    if ((mk[e0] | mk[e1] | mk[e2]) != 0 && mk[el] == 0) {
        mark[el] = 1;
        *(volatile int *)changed = 1;
    }
}

// count[t] = 1 + the marked edges of face t: its children
__global__ __launch_bounds__(256) void refine_count_kernel(const long long n_tri, const int *__restrict__ corner_edge,
                                                           const int *__restrict__ mark, int *__restrict__ count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    count[t] = 1 + mark[corner_edge[3 * t]] + mark[corner_edge[3 * t + 1]] + mark[corner_edge[3 * t + 2]];
}

// per mesh m = 0 .. n_mesh: new_before[m] = the marked edges of the meshes in front of m (a mesh's edges are contiguous:
// the first edge whose lo is a vertex of m or later, by binary search), child_before[m] = the children in front of m
__global__ __launch_bounds__(256) void refine_mesh_kernel(const int n_mesh, const long long n_edges, const long long n_tri,
                                                          const long long *__restrict__ voff, const long long *__restrict__ toff,
                                                          const int *__restrict__ edge_lo, const int *__restrict__ mark_before,
                                                          const int *__restrict__ child_off, long long *__restrict__ new_before,
                                                          long long *__restrict__ child_before) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m > n_mesh) return;
    const long long v = voff[m];
    long long lo = 0, hi = n_edges;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)edge_lo[mid] < v) lo = mid + 1; else hi = mid;
    }
    new_before[m] = mark_before[lo];
    child_before[m] = child_off[toff[m]];
}

// the vertices of the refined meshes: thread i < n_vert copies old vertex i to its new place (old vertices keep their
// mesh-local index), thread n_vert + e writes the midpoint of a marked edge e and its ends
__global__ __launch_bounds__(256) void refine_midpoint_kernel(const long long n_vert, const long long n_edges, const int n_mesh,
                                                              const long long *__restrict__ voff, const long long *__restrict__ new_before,
                                                              const double *__restrict__ xy, const int *__restrict__ edge_lo,
                                                              const int *__restrict__ edge_hi, const int *__restrict__ mark,
                                                              const int *__restrict__ mark_before, double *__restrict__ xy_out,
                                                              int *__restrict__ ends_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_vert) {
        const int m = find_segment(voff, n_mesh, i);
        const long long j = i + new_before[m];
        xy_out[2 * j] = xy[2 * i];
        xy_out[2 * j + 1] = xy[2 * i + 1];
        return;
    }
    const long long e = i - n_vert;
    if (e >= n_edges || !mark[e]) return;
    const long long lo = edge_lo[e], hi = edge_hi[e];
    const int m = find_segment(voff, n_mesh, lo);
    const long long k = mark_before[e];
    const long long j = voff[m + 1] + k;          // = new voff[m] + the mesh's old vertices + the edge's rank in the mesh
    xy_out[2 * j] = 0.5 * (xy[2 * lo] + xy[2 * hi]);
    xy_out[2 * j + 1] = 0.5 * (xy[2 * lo + 1] + xy[2 * hi + 1]);
    ends_out[2 * k] = (int)(lo - voff[m]);
    ends_out[2 * k + 1] = (int)(hi - voff[m]);
}

// the children of face t at child_off[t], mesh-local indices, parent order (the rule of DESIGN.md: the face rotated so
// that its longest edge is (a, b) with c opposite; m, p, q the midpoints of ab, bc, ca)
__global__ __launch_bounds__(256) void refine_emit_kernel(const long long n_tri, const int n_mesh, const int32_t *__restrict__ tri,
                                                          const long long *__restrict__ voff, const long long *__restrict__ toff,
                                                          const long long *__restrict__ new_before, const int *__restrict__ corner_edge,
                                                          const unsigned char *__restrict__ longest, const int *__restrict__ mark,
                                                          const int *__restrict__ mark_before, const int *__restrict__ child_off,
                                                          int *__restrict__ tri_out, int *__restrict__ parent_out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const int mesh = find_segment(toff, n_mesh, t);
    const int t0 = tri[3 * t], t1 = tri[3 * t + 1], t2 = tri[3 * t + 2];
    const int e0 = corner_edge[3 * t], e1 = corner_edge[3 * t + 1], e2 = corner_edge[3 * t + 2];
    const int l = longest[t];
    const int a = l == 0 ? t0 : l == 1 ? t1 : t2, b = l == 0 ? t1 : l == 1 ? t2 : t0, c = l == 0 ? t2 : l == 1 ? t0 : t1;
    const int eab = l == 0 ? e0 : l == 1 ? e1 : e2, ebc = l == 0 ? e1 : l == 1 ? e2 : e0, eca = l == 0 ? e2 : l == 1 ? e0 : e1;
    // mesh-local number of the new vertex of edge e: the mesh's old vertices, then its marked edges in ascending number
    const int shift = (int)(voff[mesh + 1] - voff[mesh] - new_before[mesh]);
    const long long first = child_off[t];
    const int parent = (int)(t - toff[mesh]);
    int *out = tri_out + 3 * first;
    int n = 0;
    auto put = [&](int x, int y, int z) {
        out[3 * n] = x;
        out[3 * n + 1] = y;
        out[3 * n + 2] = z;
        parent_out[first + n] = parent;
        ++n;
    };
    if (!mark[eab]) {
        put(t0, t1, t2);
        return;
    }
    const int m = shift + mark_before[eab];
    if (mark[eca]) {
        const int q = shift + mark_before[eca];
        put(a, m, q);
        put(q, m, c);
    } else {
        put(a, m, c);
    }
    if (mark[ebc]) {
        const int p = shift + mark_before[ebc];
        put(m, b, p);
        put(m, p, c);
    } else {
        put(m, b, c);
    }
}

}  // namespace padne

using namespace padne;

struct padne_refine {
    padne_ctx *owner = nullptr;
    int64_t n_mesh = 0, n_vert_out = 0, n_tri_out = 0, n_new = 0;
    // device (the owner's pool)
    double *xy = nullptr;
    int *tri = nullptr, *parent = nullptr, *ends = nullptr;
};

static void refine_free(padne_refine *r) {
    if (r == nullptr) return;
    void *blocks[] = {r->xy, r->tri, r->parent, r->ends};
    for (void *p : blocks)
        if (p) pool_free(r->owner, p);
    delete r;
}

template <typename T> static int refine_alloc(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

namespace {

struct RefineInput {
    long long n_vert = 0, n_tri = 0;
    int n_mesh = 0;
    const double *xy = nullptr;
    const int32_t *tri = nullptr;
    const long long *voff = nullptr, *toff = nullptr;
    const unsigned char *flag = nullptr;
};

// corners -> sorted keys -> heads: the edges of the batch.  Leaves the sorted keys and values and the heads with the caller
template <typename Key>
int refine_sort_corners(padne_ctx *ctx, Scratch &sc, const RefineInput &in, int key_bits, Key **key_sorted, unsigned **val_sorted,
                        int *head, int *d_err) {
    hipStream_t s = ctx->stream;
    const size_t n = 3 * (size_t)in.n_tri;
    Key *key_a = nullptr, *key_b = nullptr;
    unsigned *val_a = nullptr, *val_b = nullptr;
    PADNE_TRY(sc.alloc(&key_a, n));
    PADNE_TRY(sc.alloc(&key_b, n));
    PADNE_TRY(sc.alloc(&val_a, n));
    PADNE_TRY(sc.alloc(&val_b, n));
    hipLaunchKernelGGL(refine_corner_kernel<Key>, dim3(nblk(in.n_tri)), dim3(256), 0, s, in.n_tri, in.n_vert, in.n_mesh, in.tri,
                       in.voff, in.toff, key_a, val_a, d_err);
    PADNE_HIP_CHECK(hipGetLastError());
    // stable: the corners of an edge keep their slot order, so the sorted arrays are the same bits in every call
    size_t tmp_bytes = 0;
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_a, key_b, val_a, val_b, n, 0, key_bits, s));
    void *tmp = nullptr;
    PADNE_TRY(sc.alloc((char **)&tmp, tmp_bytes));
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, val_b, n, 0, key_bits, s));
    hipLaunchKernelGGL(refine_head_kernel<Key>, dim3(nblk((long long)n)), dim3(256), 0, s, (long long)n, (const Key *)key_b,
                       (const unsigned *)val_b, head, d_err);
    PADNE_HIP_CHECK(hipGetLastError());
    *key_sorted = key_b;
    *val_sorted = val_b;
    return PADNE_OK;
}

template <typename Key>
int refine_edges(padne_ctx *ctx, Scratch &sc, const RefineInput &in, int key_bits, int *d_err, int *corner_edge, int **edge_lo,
                 int **edge_hi, double **edge_d, int64_t *n_edges) {
    hipStream_t s = ctx->stream;
    const long long n = 3 * in.n_tri;
    Key *key = nullptr;
    unsigned *val = nullptr;
    int *head = nullptr, *before = nullptr;
    PADNE_TRY(sc.alloc(&head, (size_t)n));
    PADNE_TRY(sc.alloc(&before, (size_t)n + 1));
    PADNE_TRY(refine_sort_corners<Key>(ctx, sc, in, key_bits, &key, &val, head, d_err));
    PADNE_TRY(exclusive_scan_i32(ctx, head, before, n, n_edges));
    int h_err[REFINE_ERR_WORDS] = {0, 0, 0, 0};
    PADNE_HIP_CHECK(hipMemcpyAsync(h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_err[REFINE_BAD_INDEX]) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    if (h_err[REFINE_REPEATED]) {
        set_error("invalid argument: a face names a vertex twice");
        return PADNE_E_INVALID;
    }
    if (h_err[REFINE_NONMANIFOLD]) {
        set_error("Non-manifold mesh");
        return PADNE_E_NONMANIFOLD;
    }
    PADNE_TRY(sc.alloc(edge_lo, (size_t)*n_edges));
    PADNE_TRY(sc.alloc(edge_hi, (size_t)*n_edges));
    PADNE_TRY(sc.alloc(edge_d, (size_t)*n_edges));
    hipLaunchKernelGGL(refine_edge_kernel<Key>, dim3(nblk(n)), dim3(256), 0, s, n, in.n_vert, (const Key *)key, (const unsigned *)val,
                       (const int *)head, (const int *)before, in.xy, corner_edge, *edge_lo, *edge_hi, *edge_d);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

}  // namespace

extern "C" int padne_refine_create(padne_ctx *ctx, int64_t n_vert, const double *xy_host, int64_t n_tri, const int32_t *tri_host,
                                   int64_t n_mesh, const int64_t *mesh_vertex_offset, const int64_t *mesh_tri_offset,
                                   const uint8_t *flag_host, int64_t *new_vertex_count_out, int64_t *new_face_count_out,
                                   int64_t *counts_out, padne_refine **out) {
    PADNE_REQUIRE(ctx && out, "null argument");
    *out = nullptr;
    PADNE_REQUIRE(n_vert >= 0 && n_tri >= 0 && n_mesh > 0 && n_mesh <= 0x7fffffffLL, "sizes: at least one mesh, nothing negative");
    PADNE_REQUIRE(mesh_vertex_offset && mesh_tri_offset && new_vertex_count_out && new_face_count_out, "null argument");
    PADNE_REQUIRE(n_vert == 0 || xy_host, "null argument");
    PADNE_REQUIRE(n_tri == 0 || (tri_host && flag_host), "null argument");
    PADNE_REQUIRE(mesh_vertex_offset[0] == 0 && mesh_tri_offset[0] == 0, "offset tables must start at 0");
    PADNE_REQUIRE(mesh_vertex_offset[n_mesh] == n_vert && mesh_tri_offset[n_mesh] == n_tri, "offset tables");
    for (int64_t m = 0; m < n_mesh; ++m)
        PADNE_REQUIRE(mesh_vertex_offset[m] <= mesh_vertex_offset[m + 1] && mesh_tri_offset[m] <= mesh_tri_offset[m + 1],
                      "offset tables not monotone");
    // every index of the result fits 32 bits: at most n_vert + 3 n_tri vertices, 4 n_tri faces, 3 n_tri corner slots with a bit
    PADNE_REQUIRE(n_tri < (1LL << 28) && n_vert + 3 * n_tri < 0x7fffffffLL, "too many vertices or faces for 32-bit indices");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_refine *r = new padne_refine;
    r->owner = ctx;
    r->n_mesh = n_mesh;
    struct Guard {      // an error path hands everything back
        padne_refine *r;
        ~Guard() { refine_free(r); }
    } guard{r};
    std::vector<long long> voff(mesh_vertex_offset, mesh_vertex_offset + n_mesh + 1), toff(mesh_tri_offset, mesh_tri_offset + n_mesh + 1);
    Scratch sc(ctx);
    RefineInput in;
    in.n_vert = n_vert;
    in.n_tri = n_tri;
    in.n_mesh = (int)n_mesh;
    double *d_xy = nullptr, *edge_d = nullptr;
    int32_t *d_tri = nullptr;
    long long *d_voff = nullptr, *d_toff = nullptr, *d_new_before = nullptr, *d_child_before = nullptr;
    unsigned char *d_flag = nullptr, *d_longest = nullptr;
    int *d_err = nullptr, *d_changed = nullptr, *corner_edge = nullptr, *edge_lo = nullptr, *edge_hi = nullptr, *mark = nullptr,
        *mark_before = nullptr, *count = nullptr, *child_off = nullptr;
    PADNE_TRY(sc.alloc(&d_xy, 2 * (size_t)n_vert));
    PADNE_TRY(sc.alloc(&d_tri, 3 * (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_flag, (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_longest, (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_voff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_toff, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_new_before, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_child_before, (size_t)n_mesh + 1));
    PADNE_TRY(sc.alloc(&d_err, REFINE_ERR_WORDS));
    PADNE_TRY(sc.alloc(&d_changed, 1));
    PADNE_TRY(sc.alloc(&corner_edge, 3 * (size_t)n_tri));
    PADNE_TRY(sc.alloc(&count, (size_t)n_tri));
    PADNE_TRY(sc.alloc(&child_off, (size_t)n_tri + 1));
    PADNE_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int) * REFINE_ERR_WORDS, s));
    if (n_vert > 0) PADNE_HIP_CHECK(hipMemcpyAsync(d_xy, xy_host, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyHostToDevice, s));
    if (n_tri > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_tri, tri_host, sizeof(int32_t) * 3 * (size_t)n_tri, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_flag, flag_host, (size_t)n_tri, hipMemcpyHostToDevice, s));
    }
    PADNE_HIP_CHECK(hipMemcpyAsync(d_voff, voff.data(), sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_toff, toff.data(), sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    in.xy = d_xy;
    in.tri = d_tri;
    in.voff = d_voff;
    in.toff = d_toff;
    in.flag = d_flag;

    // ---- the edges
    int64_t n_edges = 0, n_flagged = 0, n_new = 0, n_children = 0, sweeps = 0;
    if (n_tri > 0) {
        // keys run below n_vert^2: as narrow as that allows
        const unsigned long long key_end = (unsigned long long)n_vert * (unsigned long long)n_vert;
        int key_bits = 1;
        while (key_bits < 64 && (1ull << key_bits) < key_end) ++key_bits;
        if (key_bits <= 32)
            PADNE_TRY(refine_edges<unsigned>(ctx, sc, in, key_bits, d_err, corner_edge, &edge_lo, &edge_hi, &edge_d, &n_edges));
        else
            PADNE_TRY(refine_edges<unsigned long long>(ctx, sc, in, key_bits, d_err, corner_edge, &edge_lo, &edge_hi, &edge_d, &n_edges));
    }
    PADNE_TRY(sc.alloc(&mark, (size_t)n_edges));
    PADNE_TRY(sc.alloc(&mark_before, (size_t)n_edges + 1));
    PADNE_HIP_CHECK(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)(n_edges > 0 ? n_edges : 1), s));
    PADNE_HIP_CHECK(hipMemsetAsync(mark_before, 0, sizeof(int), s));
    PADNE_HIP_CHECK(hipMemsetAsync(child_off, 0, sizeof(int), s));

    // ---- longest edges, flags, closure
    if (n_tri > 0) {
        hipLaunchKernelGGL(refine_face_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, (long long)n_tri, (const int *)corner_edge,
                           (const double *)edge_d, (const unsigned char *)d_flag, d_longest, mark);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_TRY(exclusive_scan_i32(ctx, mark, mark_before, n_edges, &n_flagged));      // (counted for the caller's record)
        // Sweeps until a whole batch of them changed nothing: the batch's first sweep then found the fixed point already.
        // No cap: the marks only grow, so at most n_edges sweeps change something.
        for (;;) {
            PADNE_HIP_CHECK(hipMemsetAsync(d_changed, 0, sizeof(int), s));
            for (int k = 0; k < kSweepsPerLook; ++k) {
                hipLaunchKernelGGL(refine_sweep_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, (long long)n_tri, (const int *)corner_edge,
                                   (const unsigned char *)d_longest, mark, d_changed);
                PADNE_HIP_CHECK(hipGetLastError());
            }
            sweeps += kSweepsPerLook;
            int h_changed = 0;
            PADNE_TRY(read_back(ctx, d_changed, sizeof(int), &h_changed));
            if (!h_changed) break;
        }
        // ---- new vertex numbers and child offsets
        PADNE_TRY(exclusive_scan_i32(ctx, mark, mark_before, n_edges, &n_new));
        hipLaunchKernelGGL(refine_count_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, (long long)n_tri, (const int *)corner_edge,
                           (const int *)mark, count);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_TRY(exclusive_scan_i32(ctx, count, child_off, n_tri, &n_children));
    }
    hipLaunchKernelGGL(refine_mesh_kernel, dim3(nblk(n_mesh + 1)), dim3(256), 0, s, (int)n_mesh, (long long)n_edges, (long long)n_tri,
                       (const long long *)d_voff, (const long long *)d_toff, (const int *)edge_lo, (const int *)mark_before,
                       (const int *)child_off, d_new_before, d_child_before);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<long long> new_before((size_t)n_mesh + 1), child_before((size_t)n_mesh + 1);
    PADNE_HIP_CHECK(hipMemcpyAsync(new_before.data(), d_new_before, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(child_before.data(), d_child_before, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyDeviceToHost, s));

    // ---- emit
    r->n_new = n_new;
    r->n_vert_out = n_vert + n_new;
    r->n_tri_out = n_children;
    PADNE_TRY(refine_alloc(ctx, &r->xy, 2 * (size_t)r->n_vert_out));
    PADNE_TRY(refine_alloc(ctx, &r->tri, 3 * (size_t)r->n_tri_out));
    PADNE_TRY(refine_alloc(ctx, &r->parent, (size_t)r->n_tri_out));
    PADNE_TRY(refine_alloc(ctx, &r->ends, 2 * (size_t)n_new));
    if (n_vert + n_edges > 0) {
        hipLaunchKernelGGL(refine_midpoint_kernel, dim3(nblk(n_vert + n_edges)), dim3(256), 0, s, (long long)n_vert, (long long)n_edges,
                           (int)n_mesh, (const long long *)d_voff, (const long long *)d_new_before, (const double *)d_xy,
                           (const int *)edge_lo, (const int *)edge_hi, (const int *)mark, (const int *)mark_before, r->xy, r->ends);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_tri > 0) {
        hipLaunchKernelGGL(refine_emit_kernel, dim3(nblk(n_tri)), dim3(256), 0, s, (long long)n_tri, (int)n_mesh, (const int32_t *)d_tri,
                           (const long long *)d_voff, (const long long *)d_toff, (const long long *)d_new_before,
                           (const int *)corner_edge, (const unsigned char *)d_longest, (const int *)mark, (const int *)mark_before,
                           (const int *)child_off, r->tri, r->parent);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t m = 0; m < n_mesh; ++m) {
        new_vertex_count_out[m] = (voff[m + 1] - voff[m]) + (new_before[m + 1] - new_before[m]);
        new_face_count_out[m] = child_before[m + 1] - child_before[m];
    }
    if (counts_out) {
        counts_out[0] = n_edges;
        counts_out[1] = n_flagged;
        counts_out[2] = n_new;
        counts_out[3] = sweeps;
    }
    guard.r = nullptr;
    *out = r;
    return PADNE_OK;
}

extern "C" int padne_refine_fetch(padne_ctx *ctx, const padne_refine *r, double *xy_out, int32_t *tri_out, int32_t *parent_out,
                                  int32_t *ends_out) {
    PADNE_REQUIRE(ctx && r, "null argument");
    PADNE_REQUIRE(ctx == r->owner, "a refinement is fetched through the context that made it");
    PADNE_REQUIRE(r->n_vert_out == 0 || xy_out, "null argument");
    PADNE_REQUIRE(r->n_tri_out == 0 || (tri_out && parent_out), "null argument");
    PADNE_REQUIRE(r->n_new == 0 || ends_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (r->n_vert_out > 0) PADNE_HIP_CHECK(hipMemcpyAsync(xy_out, r->xy, sizeof(double) * 2 * (size_t)r->n_vert_out, hipMemcpyDeviceToHost, s));
    if (r->n_tri_out > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(tri_out, r->tri, sizeof(int32_t) * 3 * (size_t)r->n_tri_out, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(parent_out, r->parent, sizeof(int32_t) * (size_t)r->n_tri_out, hipMemcpyDeviceToHost, s));
    }
    if (r->n_new > 0) PADNE_HIP_CHECK(hipMemcpyAsync(ends_out, r->ends, sizeof(int32_t) * 2 * (size_t)r->n_new, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_refine_destroy(padne_refine *r) {
    if (r == nullptr) return PADNE_OK;
    if (r->owner) {
        (void)hipSetDevice(r->owner->device);
        (void)hipStreamSynchronize(r->owner->stream);
    }
    refine_free(r);
    return PADNE_OK;
}
