// Heat conduction between stacked layers through the dielectric ("Stack").  No reference counterpart.
//
// The user names pairs of layers (a, b) with an areal conductance g_ab [W/(K length^2)].  The coupling is a sum of ordinary
// two-terminal thermal conductances, generated from both sides of every pair with half weight each:
//
//   for side (s -> t) in ((a -> b), (b -> a)), for every vertex v of a mesh of layer s, at q = xy[v]:
//     f        = the owner face of q among the meshes of layer t, by the sampler's rule (locate.hpp); none: nothing
//     lambda_k = o_k / s, s = (o_a + o_b) + o_c, the sampler's weights of the three corners of f
//     c_k      = ((0.5 g_ab) M_v) lambda_k;  c_k == 0: nothing;  else a link of conductance c_k between v and tri[f][k]
//
//   G_ij (i != j) = -(the sum of the links between i and j)     (at most one from each side: two terms, no order)
//   G_ii          = the sum over the stored partners j of row i, ascending, of (-G_ij), from 0.0
//   A'_ij         = A_ij + G_ij, one rounded add where both are stored, the stored one otherwise
//
// G is symmetric, annihilates constants and has no positive off-diagonal: A' = A + G stays an M-matrix, and the film loss
// still equals the heat put in.  padne_thermal_create_stacked replaces the matrix of a thermal handle by A' before anybody
// has looked at it, so the block solve, the electro-thermal loop and the transient's S = A + C/dt work on A' as they are.
//
// Four stages, every kernel a gather or a stream bound by memory, one thread per item in workgroups of 256:
//   1. the bin grid of every layer a pair names, over the meshes the system keeps on the device (sample.hip's index build);
//   2. locate: one thread per (side, vertex) writes its owner, three weights and three conductances at fixed places, and the
//      two directed entries (v, u, c), (u, v, c) of every link -- no compaction, no atomics;
//   3. G: the directed entries grouped by (row, column) with a stable radix sort, the runs summed front to back;
//   4. A': per row the merge of two ascending rows, counted, scanned and filled.
// No floating-point atomics; the flows go through the fixed-order tile reductions of error.hpp: two calls give the same
// bits.  Compiled with -ffp-contract=off: the expressions round as written, tests/stack_ref.py reproduces them.
#include "locate.hpp"
#include "thermal.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <string>
#include <vector>

namespace padne {

void stack_free(padne_ctx *ctx, padne_stack *st) {
    if (st == nullptr) return;
    for (void *p : {(void *)st->owner, (void *)st->vertex, (void *)st->mesh_layer_dev, (void *)st->vertex_layer, (void *)st->weight,
                    (void *)st->cond, (void *)st->gptr, (void *)st->gcol, (void *)st->gval, (void *)st->gdiag})
        if (p != nullptr) pool_free(ctx, p);
    delete st;
}

// ---- stage 1: the bounding box of every mesh -------------------------------------------------------------------------------
constexpr int kBoxParts = 64;          // workgroups per mesh: a mesh of a million vertices keeps every CU busy

// box[m][part] = (min x, min y, max x, max y) over the vertices of mesh m = blockIdx.x that part = blockIdx.y strides over
// (+-infinity without any); the host joins the parts.  Minima and maxima do not depend on the order they are taken in.
// Also vertex_layer[v] = the layer of the mesh of v
__global__ __launch_bounds__(256) void stack_box_kernel(const long long *__restrict__ voff, const double *__restrict__ xy,
                                                        const int *__restrict__ mesh_layer, double *__restrict__ box,
                                                        int *__restrict__ vertex_layer) {
    __shared__ double red[4][4];
    const int m = blockIdx.x;
    const int layer = mesh_layer[m];
    double lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    for (long long v = voff[m] + (long long)blockIdx.y * 256 + threadIdx.x; v < voff[m + 1]; v += (long long)kBoxParts * 256) {
        const double x = xy[2 * v], y = xy[2 * v + 1];
        lx = fmin(lx, x);
        ly = fmin(ly, y);
        hx = fmax(hx, x);
        hy = fmax(hy, y);
        vertex_layer[v] = layer;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lx = fmin(lx, __shfl_down(lx, off, 64));
        ly = fmin(ly, __shfl_down(ly, off, 64));
        hx = fmax(hx, __shfl_down(hx, off, 64));
        hy = fmax(hy, __shfl_down(hy, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = lx;
        red[threadIdx.x >> 6][1] = ly;
        red[threadIdx.x >> 6][2] = hx;
        red[threadIdx.x >> 6][3] = hy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lx = fmin(lx, red[w][0]);
            ly = fmin(ly, red[w][1]);
            hx = fmax(hx, red[w][2]);
            hy = fmax(hy, red[w][3]);
        }
        double *out = box + 4 * ((long long)m * kBoxParts + blockIdx.y);
        out[0] = lx;
        out[1] = ly;
        out[2] = hx;
        out[3] = hy;
    }
}

// ---- stage 2: locate -------------------------------------------------------------------------------------------------------
// Slot q belongs to segment e = (one side, one mesh of the side's source layer): vertex v = seg_v0[e] + (q - seg_q0[e]).
// Writes the slot and its six directed entries: key = row << 32 | column, val = c; a link that does not exist gets the key
// n_pot << 32, which sorts behind every row
__global__ __launch_bounds__(256) void stack_locate_kernel(const long long n_query, const int n_seg, const long long *__restrict__ seg_q0,
                                                           const long long *__restrict__ seg_v0, const int *__restrict__ seg_side,
                                                           const int *__restrict__ side_target, const double *__restrict__ side_half_g,
                                                           const LayerGrid *__restrict__ grids, const int *__restrict__ bin_off,
                                                           const int *__restrict__ bin_face, const int *__restrict__ gtri,
                                                           const double *__restrict__ xy, const double *__restrict__ Mv,
                                                           const long long n_pot, int *__restrict__ owner_out,
                                                           int *__restrict__ vertex_out, double *__restrict__ weight_out,
                                                           double *__restrict__ cond_out, unsigned long long *__restrict__ key,
                                                           double *__restrict__ val) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_query) return;
    const int e = find_segment(seg_q0, n_seg, q);
    const long long v = seg_v0[e] + (q - seg_q0[e]);
    const int side = seg_side[e];
    const LayerGrid g = grids[side_target[side]];
    double o[3];
    unsigned long long n_tested = 0;
    const int f = locate_owner(g, bin_off, bin_face, gtri, xy, xy[2 * v], xy[2 * v + 1], o[0], o[1], o[2], n_tested);
    const bool found = f != kNoOwner;
    const double s = (o[0] + o[1]) + o[2];
    const double gm = side_half_g[side] * Mv[v];
    owner_out[q] = found ? f : -1;
    vertex_out[q] = (int)v;
    const unsigned long long none = (unsigned long long)n_pot << 32;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = found ? o[k] / s : 0.0;
        const double c = found ? gm * w : 0.0;
        weight_out[3 * q + k] = w;
        cond_out[3 * q + k] = c;
        const bool link = found && c != 0.0;
        const unsigned long long u = link ? (unsigned long long)gtri[3 * (long long)f + k] : 0ull;
        key[6 * q + 2 * k] = link ? ((unsigned long long)v << 32) | u : none;
        key[6 * q + 2 * k + 1] = link ? (u << 32) | (unsigned long long)v : none;
        val[6 * q + 2 * k] = c;
        val[6 * q + 2 * k + 1] = c;
    }
}

// ---- stage 3: G ------------------------------------------------------------------------------------------------------------
// head[i] = 1 where sorted entry i starts the run of a (row, column) that exists
__global__ __launch_bounds__(256) void stack_head_kernel(const long long n, const long long n_pot,
                                                         const unsigned long long *__restrict__ key, int *__restrict__ head) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    head[i] = (long long)(k >> 32) < n_pot && (i == 0 || key[i - 1] != k) ? 1 : 0;
}

// the run that starts at i becomes stored entry pos[i] of G: the sum of its conductances front to back, negated
__global__ __launch_bounds__(256) void stack_compact_kernel(const long long n, const unsigned long long *__restrict__ key,
                                                            const double *__restrict__ val, const int *__restrict__ head,
                                                            const int *__restrict__ pos, int *__restrict__ grow,
                                                            int *__restrict__ gcol, double *__restrict__ gval) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i]) return;
    const unsigned long long k = key[i];
    double sum = val[i];
    for (long long e = i + 1; e < n && key[e] == k; ++e) sum = sum + val[e];
    const int at = pos[i];
    grow[at] = (int)(k >> 32);
    gcol[at] = (int)(k & 0xffffffffull);
    gval[at] = -sum;
}

// gptr[i] = the first stored entry of a row >= i, i = 0 .. n_pot
__global__ __launch_bounds__(256) void stack_ptr_kernel(const long long n_pot, const long long nnz, const int *__restrict__ grow,
                                                        int *__restrict__ gptr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > n_pot) return;
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)grow[mid] < i) lo = mid + 1; else hi = mid;
    }
    gptr[i] = (int)lo;
}

// gdiag[i] = the sum of (-G_ij) along row i, from 0.0
__global__ __launch_bounds__(256) void stack_diag_kernel(const long long n_pot, const int *__restrict__ gptr,
                                                         const double *__restrict__ gval, double *__restrict__ gdiag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    double d = 0.0;
    for (int e = gptr[i], e1 = gptr[i + 1]; e < e1; ++e) d = d + (-gval[e]);
    gdiag[i] = d;
}

// ---- stage 4: A' -----------------------------------------------------------------------------------------------------------
// The merge of row i of A (ascending, with its diagonal) and row i of G (ascending, no diagonal).  FILL = false: count[i] =
// the entries of the union; FILL = true: they are written from out_ptr[i] on, A_ij + G_ij where both are stored, and the
// diagonal of a row G reaches becomes A_ii + gdiag[i]
template <bool FILL>
__global__ __launch_bounds__(256) void stack_merge_kernel(const long long n_pot, const int32_t *__restrict__ aptr,
                                                          const int32_t *__restrict__ acol, const double *__restrict__ aval,
                                                          const int *__restrict__ gptr, const int *__restrict__ gcol,
                                                          const double *__restrict__ gval, const double *__restrict__ gdiag,
                                                          int *__restrict__ count, const int32_t *__restrict__ out_ptr,
                                                          int32_t *__restrict__ out_col, double *__restrict__ out_val) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pot) return;
    int ea = aptr[i], eg = gptr[i];
    const int ea1 = aptr[i + 1], eg1 = gptr[i + 1];
    const bool reached = eg1 > eg;
    int n = 0;
    int at = FILL ? out_ptr[i] : 0;
    while (ea < ea1 || eg < eg1) {
        const int ca = ea < ea1 ? acol[ea] : 0x7fffffff, cg = eg < eg1 ? gcol[eg] : 0x7fffffff;
        if (FILL) {
            double a;
            if (ca == cg) a = aval[ea] + gval[eg];
            else if (ca < cg) a = reached && ca == i ? aval[ea] + gdiag[i] : aval[ea];
            else a = gval[eg];
            out_col[at] = ca < cg ? ca : cg;
            out_val[at] = a;
            ++at;
        }
        ++n;
        if (ca <= cg) ++ea;
        if (cg <= ca) ++eg;
    }
    if (!FILL) count[i] = n;
}

// ---- flows -----------------------------------------------------------------------------------------------------------------
// Per tile (256 vertices of one mesh), pair p and column c: tile[(c n_pair + p)][b] = the sum over the tile's vertices i and
// their partners j in layer pair_b[p], ascending, of (-G_ij)(theta[c][i] - theta[c][j]) for the tiles of a mesh of layer
// pair_a[p], 0 for the others; column n_cols stands for the area: the terms are (-G_ij).  Sums in the order of error.hpp
__global__ __launch_bounds__(256) void stack_flow_kernel(const int n_mesh, const long long *__restrict__ vtile_off,
                                                         const long long *__restrict__ voff, const long long n_pot,
                                                         const long long n_blocks, const int n_cols, const int n_pair,
                                                         const int *__restrict__ pair_a, const int *__restrict__ pair_b,
                                                         const int *__restrict__ mesh_layer,
                                                         const int *__restrict__ vertex_layer, const int *__restrict__ gptr,
                                                         const int *__restrict__ gcol, const double *__restrict__ gval,
                                                         const double *__restrict__ theta, double *__restrict__ tile) {
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
        for (int c = 0; c <= n_cols; ++c) {
            double acc = 0.0;
            if (mine) {
                const double *th = theta + (long long)c * n_pot;
                const double ti = c < n_cols && live ? th[v] : 0.0;
                for (int e = e0; e < e1; ++e) {
                    const long long j = gcol[e];
                    if (vertex_layer[j] != lb) continue;
                    acc = c < n_cols ? acc + (-gval[e]) * (ti - th[j]) : acc + (-gval[e]);
                }
            }
            acc = error_wave_sum(acc);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) tile[((long long)c * n_pair + p) * n_blocks + b] = error_sum4(red);
            __syncthreads();
        }
    }
}

// out[y][m] = the sum of tile[y][..] over the tiles of mesh m = blockIdx.x, y = blockIdx.y: strided partial sums, then the
// wave and workgroup order of error.hpp
__global__ __launch_bounds__(256) void stack_fold_kernel(const int n_mesh, const long long n_blocks,
                                                         const long long *__restrict__ vtile_off, const double *__restrict__ tile,
                                                         double *__restrict__ out) {
    __shared__ double red[4];
    const int m = blockIdx.x;
    const long long at = (long long)blockIdx.y * n_blocks;
    double s = 0.0;
    for (long long i = vtile_off[m] + threadIdx.x; i < vtile_off[m + 1]; i += 256) s += tile[at + i];
    s = error_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(long long)blockIdx.y * n_mesh + m] = error_sum4(red);
}

template <typename T> static int stack_keep(padne_ctx *ctx, T **out, size_t count) {
    *out = (T *)pool_alloc(ctx, sizeof(T) * (count ? count : 1));
    return *out ? PADNE_OK : PADNE_E_NOMEM;
}

template <typename T> static int stack_upload(padne_ctx *ctx, Scratch &sc, T **out, const std::vector<T> &host) {
    PADNE_TRY(sc.alloc(out, host.size()));
    if (!host.empty())
        PADNE_HIP_CHECK(hipMemcpyAsync(*out, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, ctx->stream));
    return PADNE_OK;
}

// Stages 1 to 4 on a fresh thermal handle: th->stack filled, th->A replaced by A'
static int stack_build(padne_ctx *ctx, padne_thermal *th) {
    padne_stack *st = th->stack;
    hipStream_t s = ctx->stream;
    const ErrorMesh M = error_mesh_of(th->L);
    const int n_mesh = th->n_mesh, n_layer = st->n_layer;
    const long long n_pot = th->n_pot, n_tri = th->n_tri;
    PADNE_TRY(stack_keep(ctx, &st->mesh_layer_dev, (size_t)n_mesh));
    PADNE_HIP_CHECK(hipMemcpyAsync(st->mesh_layer_dev, st->mesh_layer.data(), sizeof(int) * (size_t)n_mesh, hipMemcpyHostToDevice, s));
    // the sides of the pairs that conduct, their segments (side, mesh of the source layer) and slots
    std::vector<int> side_target, seg_side;
    std::vector<double> side_half_g;
    std::vector<long long> seg_q0, seg_v0;
    st->q_side_off.assign(1, 0);
    long long n_query = 0;
    for (int p = 0; p < st->n_pair; ++p) {
        if (st->pair_g[(size_t)p] == 0.0) continue;                // no pair
        for (int d = 0; d < 2; ++d) {
            const int from = d == 0 ? st->pair_a[(size_t)p] : st->pair_b[(size_t)p];
            const int side = (int)side_target.size();
            side_target.push_back(d == 0 ? st->pair_b[(size_t)p] : st->pair_a[(size_t)p]);
            side_half_g.push_back(0.5 * st->pair_g[(size_t)p]);
            for (int m = 0; m < n_mesh; ++m) {
                if (st->mesh_layer[(size_t)m] != from || th->voff[(size_t)m + 1] == th->voff[(size_t)m]) continue;
                seg_q0.push_back(n_query);
                seg_v0.push_back(th->voff[(size_t)m]);
                seg_side.push_back(side);
                n_query += th->voff[(size_t)m + 1] - th->voff[(size_t)m];
            }
            st->q_side_off.push_back(n_query);
        }
    }
    seg_q0.push_back(n_query);
    st->n_side = (int)side_target.size();
    st->n_query = n_query;
    const int n_seg = (int)seg_side.size();
    PADNE_REQUIRE(6 * n_query <= 0x7fffffffLL, "too many (side, vertex) pairs for 32-bit link lists");
    PADNE_TRY(stack_keep(ctx, &st->owner, (size_t)n_query));
    PADNE_TRY(stack_keep(ctx, &st->vertex, (size_t)n_query));
    PADNE_TRY(stack_keep(ctx, &st->weight, 3 * (size_t)n_query));
    PADNE_TRY(stack_keep(ctx, &st->cond, 3 * (size_t)n_query));
    PADNE_TRY(stack_keep(ctx, &st->vertex_layer, (size_t)th->n_vert));
    PADNE_TRY(stack_keep(ctx, &st->gptr, (size_t)n_pot + 1));
    PADNE_TRY(stack_keep(ctx, &st->gdiag, (size_t)n_pot));
    if (n_query == 0) {                                            // nothing couples: G = 0, A' = A as it stands
        PADNE_HIP_CHECK(hipMemsetAsync(st->gptr, 0, sizeof(int) * ((size_t)n_pot + 1), s));
        PADNE_HIP_CHECK(hipMemsetAsync(st->gdiag, 0, sizeof(double) * (size_t)(n_pot > 0 ? n_pot : 1), s));
        PADNE_TRY(stack_keep(ctx, &st->gcol, 0));
        PADNE_TRY(stack_keep(ctx, &st->gval, 0));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
        return PADNE_OK;
    }
    const long long n_ent = 6 * n_query;
    Scratch sc(ctx);
    // ---- 1: global corners, bounding boxes, the bin grid of every layer
    int *d_gtri = nullptr, *d_bad = nullptr;
    double *d_box = nullptr;
    PADNE_TRY(sc.alloc(&d_gtri, 3 * (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_TRY(sc.alloc(&d_box, 4 * (size_t)n_mesh * kBoxParts));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    PADNE_TRY(locate_global_corners(ctx, n_tri, M.tri, n_mesh, M.voff, M.toff, d_gtri, d_bad));
    PADNE_REQUIRE(n_mesh <= 0x7fffffff / kBoxParts, "too many meshes for one launch");
    hipLaunchKernelGGL(stack_box_kernel, dim3((unsigned)n_mesh, kBoxParts), dim3(256), 0, s, M.voff, M.xy,
                       (const int *)st->mesh_layer_dev, d_box, st->vertex_layer);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<double> box(4 * (size_t)n_mesh * kBoxParts);
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(box.data(), d_box, sizeof(double) * box.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    PADNE_REQUIRE(!h_bad, "triangle index out of range");
    std::vector<double> lo(2 * (size_t)n_layer, INFINITY), hi(2 * (size_t)n_layer, -INFINITY);
    std::vector<int64_t> layer_faces((size_t)n_layer, 0), layer_entries((size_t)n_layer, 0);
    // only the layers a conducting pair names are searched: the meshes of the others are left out of the index
    std::vector<char> coupled((size_t)n_layer, 0);
    for (int t : side_target) coupled[(size_t)t] = 1;
    std::vector<int> bin_layer((size_t)n_mesh);
    for (int m = 0; m < n_mesh; ++m) {
        const size_t l = (size_t)st->mesh_layer[(size_t)m];
        bin_layer[(size_t)m] = coupled[l] ? (int)l : -1;
        if (!coupled[l]) continue;
        layer_faces[l] += th->toff[(size_t)m + 1] - th->toff[(size_t)m];
        for (size_t part = 0; part < (size_t)kBoxParts; ++part)
            for (int k = 0; k < 2; ++k) {
                lo[2 * l + k] = std::fmin(lo[2 * l + k], box[4 * ((size_t)m * kBoxParts + part) + k]);
                hi[2 * l + k] = std::fmax(hi[2 * l + k], box[4 * ((size_t)m * kBoxParts + part) + 2 + k]);
            }
    }
    int *d_bin_layer = nullptr;
    PADNE_TRY(stack_upload(ctx, sc, &d_bin_layer, bin_layer));
    for (size_t l = 0; l < (size_t)n_layer; ++l) {
        PADNE_REQUIRE(!(lo[2 * l] <= hi[2 * l]) || (std::isfinite(lo[2 * l]) && std::isfinite(lo[2 * l + 1]) &&
                                                     std::isfinite(hi[2 * l]) && std::isfinite(hi[2 * l + 1])),
                      "vertex coordinates must be finite");
        if (!(lo[2 * l] <= hi[2 * l])) lo[2 * l] = lo[2 * l + 1] = hi[2 * l] = hi[2 * l + 1] = 0.0;      // a layer without vertices
    }
    std::vector<LayerGrid> grid((size_t)n_layer);
    struct Bins {
        padne_ctx *ctx;
        int *off = nullptr, *face = nullptr;
        ~Bins() {
            if (off) pool_free(ctx, off);
            if (face) pool_free(ctx, face);
        }
    } bins{ctx};
    PADNE_TRY(locate_build_bins(ctx, n_layer, lo.data(), hi.data(), 0, layer_faces, n_tri, d_gtri, M.xy, n_mesh, M.toff,
                                d_bin_layer, grid, layer_entries, &bins.off, &bins.face));
    // ---- 2: locate
    long long *d_q0 = nullptr, *d_v0 = nullptr;
    int *d_seg_side = nullptr, *d_target = nullptr;
    double *d_half_g = nullptr;
    LayerGrid *d_grid = nullptr;
    unsigned long long *key_a = nullptr, *key_b = nullptr;
    double *val_a = nullptr, *val_b = nullptr;
    PADNE_TRY(stack_upload(ctx, sc, &d_q0, seg_q0));
    PADNE_TRY(stack_upload(ctx, sc, &d_v0, seg_v0));
    PADNE_TRY(stack_upload(ctx, sc, &d_seg_side, seg_side));
    PADNE_TRY(stack_upload(ctx, sc, &d_target, side_target));
    PADNE_TRY(stack_upload(ctx, sc, &d_half_g, side_half_g));
    PADNE_TRY(stack_upload(ctx, sc, &d_grid, grid));
    PADNE_TRY(sc.alloc(&key_a, (size_t)n_ent));
    PADNE_TRY(sc.alloc(&key_b, (size_t)n_ent));
    PADNE_TRY(sc.alloc(&val_a, (size_t)n_ent));
    PADNE_TRY(sc.alloc(&val_b, (size_t)n_ent));
    hipLaunchKernelGGL(stack_locate_kernel, dim3(nblk(n_query)), dim3(256), 0, s, n_query, n_seg, (const long long *)d_q0,
                       (const long long *)d_v0, (const int *)d_seg_side, (const int *)d_target, (const double *)d_half_g,
                       (const LayerGrid *)d_grid, (const int *)bins.off, (const int *)bins.face, (const int *)d_gtri, M.xy,
                       (const double *)th->Mv, n_pot, st->owner, st->vertex, st->weight, st->cond, key_a, val_a);
    PADNE_HIP_CHECK(hipGetLastError());
    // ---- 3: G.  Stable: equal (row, column) keep the order of the slots
    int key_bits = 33;
    while (key_bits < 64 && (1ll << (key_bits - 32)) <= n_pot) ++key_bits;      // rows run to n_pot inclusive
    size_t tmp_bytes = 0;
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_a, key_b, val_a, val_b, (size_t)n_ent, 0, key_bits, s));
    void *tmp = nullptr;
    PADNE_TRY(sc.alloc((char **)&tmp, tmp_bytes));
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, val_b, (size_t)n_ent, 0, key_bits, s));
    int *d_head = nullptr, *d_pos = nullptr, *d_grow = nullptr;
    PADNE_TRY(sc.alloc(&d_head, (size_t)n_ent));
    PADNE_TRY(sc.alloc(&d_pos, (size_t)n_ent + 1));
    hipLaunchKernelGGL(stack_head_kernel, dim3(nblk(n_ent)), dim3(256), 0, s, n_ent, n_pot, (const unsigned long long *)key_b, d_head);
    PADNE_HIP_CHECK(hipGetLastError());
    int64_t nnz = 0;
    PADNE_TRY(exclusive_scan_i32(ctx, d_head, d_pos, n_ent, &nnz));
    st->nnz = nnz;
    PADNE_TRY(stack_keep(ctx, &st->gcol, (size_t)nnz));
    PADNE_TRY(stack_keep(ctx, &st->gval, (size_t)nnz));
    PADNE_TRY(sc.alloc(&d_grow, (size_t)nnz));
    hipLaunchKernelGGL(stack_compact_kernel, dim3(nblk(n_ent)), dim3(256), 0, s, n_ent, (const unsigned long long *)key_b,
                       (const double *)val_b, (const int *)d_head, (const int *)d_pos, d_grow, st->gcol, st->gval);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(stack_ptr_kernel, dim3(nblk(n_pot + 1)), dim3(256), 0, s, n_pot, (long long)nnz, (const int *)d_grow, st->gptr);
    PADNE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(stack_diag_kernel, dim3(nblk(n_pot)), dim3(256), 0, s, n_pot, (const int *)st->gptr, (const double *)st->gval,
                       st->gdiag);
    PADNE_HIP_CHECK(hipGetLastError());
    // ---- 4: A' on the union pattern, into the arrays of the handle's matrix (nobody has derived anything from A yet)
    padne_csr *A = th->A;
    int *d_count = nullptr;
    PADNE_TRY(sc.alloc(&d_count, (size_t)n_pot));
    hipLaunchKernelGGL(stack_merge_kernel<false>, dim3(nblk(n_pot)), dim3(256), 0, s, n_pot, (const int32_t *)A->rowptr,
                       (const int32_t *)A->cols, (const double *)A->vals, (const int *)st->gptr, (const int *)st->gcol,
                       (const double *)st->gval, (const double *)st->gdiag, d_count, (const int32_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr);
    PADNE_HIP_CHECK(hipGetLastError());
    Scratch fresh(ctx);
    int32_t *n_ptr = nullptr, *n_col = nullptr;
    double *n_val = nullptr;
    PADNE_TRY(fresh.alloc(&n_ptr, (size_t)n_pot + 1));
    int64_t total = 0;
    PADNE_TRY(exclusive_scan_i32(ctx, d_count, n_ptr, n_pot, &total));
    PADNE_REQUIRE(total < (int64_t)2147483647 - kPadNnz, "matrix too large for int32 indices");
    PADNE_TRY(fresh.alloc(&n_col, (size_t)total + kPadNnz));
    PADNE_TRY(fresh.alloc(&n_val, (size_t)total + kPadNnz));
    hipLaunchKernelGGL(stack_merge_kernel<true>, dim3(nblk(n_pot)), dim3(256), 0, s, n_pot, (const int32_t *)A->rowptr,
                       (const int32_t *)A->cols, (const double *)A->vals, (const int *)st->gptr, (const int *)st->gcol,
                       (const double *)st->gval, (const double *)st->gdiag, (int *)nullptr, (const int32_t *)n_ptr, n_col, n_val);
    PADNE_HIP_CHECK(hipGetLastError());
    csr_invalidate_values(A);
    pool_free(ctx, A->rowptr);
    pool_free(ctx, A->cols);
    pool_free(ctx, A->vals);
    A->rowptr = n_ptr;
    A->cols = n_col;
    A->vals = n_val;
    A->nnz = total;
    fresh.disown(n_ptr);
    fresh.disown(n_col);
    fresh.disown(n_val);
    PADNE_TRY(csr_shrink_nnz(ctx, A, total));                      // the padding behind the real end (csr_alloc)
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

static int stack_require(const char *entry, padne_ctx *ctx, const padne_thermal *th) {
    PADNE_TRY(thermal_require(entry, ctx, th));
    PADNE_REQUIRE(th->stack != nullptr, (std::string(entry) + ": the handle was not made by padne_thermal_create_stacked").c_str());
    return PADNE_OK;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_thermal_create_stacked(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int32_t n_mesh,
                                            const double *kappa, const double *film, int64_t n_link, const int64_t *link_a,
                                            const int64_t *link_b, const double *link_g, int32_t n_layer,
                                            const int32_t *mesh_layer, int32_t n_pair, const int32_t *pair_a,
                                            const int32_t *pair_b, const double *pair_g, padne_thermal **out) {
    PADNE_REQUIRE(ctx && out, "null argument");
    PADNE_REQUIRE(n_layer >= 1 && n_pair >= 0 && n_mesh >= 0, "at least one layer, no negative count");
    PADNE_REQUIRE(mesh_layer != nullptr || n_mesh == 0, "null argument");
    PADNE_REQUIRE(n_pair == 0 || (pair_a && pair_b && pair_g), "null argument");
    for (int32_t m = 0; m < n_mesh; ++m) PADNE_REQUIRE(mesh_layer[m] >= 0 && mesh_layer[m] < n_layer, "mesh layer out of range");
    for (int32_t p = 0; p < n_pair; ++p) {
        PADNE_REQUIRE(pair_a[p] >= 0 && pair_a[p] < n_layer && pair_b[p] >= 0 && pair_b[p] < n_layer, "pair layer out of range");
        PADNE_REQUIRE(pair_a[p] != pair_b[p], "a pair names two different layers");
        PADNE_REQUIRE(std::isfinite(pair_g[p]) && pair_g[p] >= 0.0, "a pair's conductance must be finite and not negative");
        for (int32_t q = 0; q < p; ++q)
            PADNE_REQUIRE(!((pair_a[q] == pair_a[p] && pair_b[q] == pair_b[p]) || (pair_a[q] == pair_b[p] && pair_b[q] == pair_a[p])),
                          "a pair of layers is named once");
    }
    padne_thermal *th = nullptr;
    PADNE_TRY(padne_thermal_create(ctx, L, n_potential, n_mesh, kappa, film, n_link, link_a, link_b, link_g, &th));
    struct Guard {
        padne_thermal *th;
        ~Guard() { if (th) padne_thermal_destroy(th); }
    } guard{th};
    padne_stack *st = new padne_stack;
    th->stack = st;
    st->n_layer = n_layer;
    st->n_pair = n_pair;
    st->mesh_layer.assign(mesh_layer, mesh_layer + n_mesh);
    st->pair_a.assign(pair_a, pair_a + n_pair);
    st->pair_b.assign(pair_b, pair_b + n_pair);
    st->pair_g.assign(pair_g, pair_g + n_pair);
    PADNE_TRY(stack_build(ctx, th));
    guard.th = nullptr;
    *out = th;
    return PADNE_OK;
}

extern "C" int padne_thermal_stack_sizes(const padne_thermal *th, int64_t *counts_out) {
    PADNE_REQUIRE(th && counts_out, "null argument");
    PADNE_REQUIRE(th->stack != nullptr, "the handle was not made by padne_thermal_create_stacked");
    counts_out[0] = th->stack->n_pair;
    counts_out[1] = th->stack->n_side;
    counts_out[2] = th->stack->n_query;
    counts_out[3] = th->stack->nnz;
    return PADNE_OK;
}

extern "C" int padne_thermal_stack_links(padne_ctx *ctx, const padne_thermal *th, int64_t n_query, int64_t *side_offset_out,
                                         int32_t *vertex_out, int32_t *owner_out, double *weight_out, double *cond_out) {
    PADNE_TRY(stack_require("padne_thermal_stack_links", ctx, th));
    const padne_stack *st = th->stack;
    PADNE_REQUIRE(n_query == st->n_query, "n_query must be that of padne_thermal_stack_sizes");
    PADNE_REQUIRE(side_offset_out != nullptr, "null argument");
    for (size_t i = 0; i < st->q_side_off.size(); ++i) side_offset_out[i] = st->q_side_off[i];
    if (n_query == 0) return PADNE_OK;
    PADNE_REQUIRE(vertex_out && owner_out && weight_out && cond_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PADNE_HIP_CHECK(hipMemcpyAsync(vertex_out, st->vertex, sizeof(int) * (size_t)n_query, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(owner_out, st->owner, sizeof(int) * (size_t)n_query, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(weight_out, st->weight, sizeof(double) * 3 * (size_t)n_query, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(cond_out, st->cond, sizeof(double) * 3 * (size_t)n_query, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_thermal_stack_matrix(padne_ctx *ctx, const padne_thermal *th, int64_t nnz, int32_t *indptr_out,
                                          int32_t *indices_out, double *data_out, double *diag_out) {
    PADNE_TRY(stack_require("padne_thermal_stack_matrix", ctx, th));
    const padne_stack *st = th->stack;
    PADNE_REQUIRE(nnz == st->nnz, "nnz must be that of padne_thermal_stack_sizes");
    PADNE_REQUIRE(indptr_out && (th->n_pot == 0 || diag_out) && (nnz == 0 || (indices_out && data_out)), "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PADNE_HIP_CHECK(hipMemcpyAsync(indptr_out, st->gptr, sizeof(int) * ((size_t)th->n_pot + 1), hipMemcpyDeviceToHost, s));
    if (th->n_pot > 0) PADNE_HIP_CHECK(hipMemcpyAsync(diag_out, st->gdiag, sizeof(double) * (size_t)th->n_pot, hipMemcpyDeviceToHost, s));
    if (nnz > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(indices_out, st->gcol, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(data_out, st->gval, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    return PADNE_OK;
}

extern "C" int padne_thermal_stack_flows(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *flow_out, double *area_out) {
    PADNE_TRY(stack_require("padne_thermal_stack_flows", ctx, th));
    const padne_stack *st = th->stack;
    PADNE_REQUIRE(n_cols >= 0, "negative column count");
    PADNE_REQUIRE(n_cols == 0 || (th->solved && n_cols == th->n_cols), "padne_thermal_stack_flows follows a solve of as many columns");
    const int n_pair = st->n_pair, n_mesh = th->n_mesh;
    if (n_pair == 0) return PADNE_OK;
    PADNE_REQUIRE((n_cols == 0 || flow_out) && area_out, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const std::vector<long long> vtile = thermal_tiles(th->voff);
    const long long n_vb = vtile[(size_t)n_mesh];
    PADNE_REQUIRE(n_vb <= 0x7fffffffLL, "too many tiles for one launch");
    const size_t ny = ((size_t)n_cols + 1) * (size_t)n_pair;
    PADNE_REQUIRE(ny <= 65535, "too many columns times pairs for one launch");
    std::vector<double> mesh_sum(ny * (size_t)n_mesh, 0.0);
    if (n_vb > 0) {
        const ErrorMesh M = error_mesh_of(th->L);
        Scratch sc(ctx);
        long long *d_vtile = nullptr;
        int *d_a = nullptr, *d_b = nullptr;
        double *d_tile = nullptr, *d_out = nullptr;
        PADNE_TRY(stack_upload(ctx, sc, &d_vtile, vtile));
        PADNE_TRY(stack_upload(ctx, sc, &d_a, st->pair_a));
        PADNE_TRY(stack_upload(ctx, sc, &d_b, st->pair_b));
        PADNE_TRY(sc.alloc(&d_tile, ny * (size_t)n_vb));
        PADNE_TRY(sc.alloc(&d_out, ny * (size_t)n_mesh));
        hipLaunchKernelGGL(stack_flow_kernel, dim3((unsigned)n_vb), dim3(256), 0, s, n_mesh, (const long long *)d_vtile, M.voff,
                           th->n_pot, n_vb, (int)n_cols, n_pair, (const int *)d_a, (const int *)d_b, (const int *)st->mesh_layer_dev,
                           (const int *)st->vertex_layer, (const int *)st->gptr, (const int *)st->gcol, (const double *)st->gval,
                           (const double *)th->theta, d_tile);
        PADNE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(stack_fold_kernel, dim3((unsigned)n_mesh, (unsigned)ny), dim3(256), 0, s, n_mesh, n_vb,
                           (const long long *)d_vtile, (const double *)d_tile, d_out);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(mesh_sum.data(), d_out, sizeof(double) * mesh_sum.size(), hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
    }
    // the meshes of layer a in ascending order, from 0.0; the area is that sum of (-G_ij) over g (0 for a pair without g)
    for (int c = 0; c <= n_cols; ++c)
        for (int p = 0; p < n_pair; ++p) {
            double sum = 0.0;
            for (int m = 0; m < n_mesh; ++m)
                if (st->mesh_layer[(size_t)m] == st->pair_a[(size_t)p]) sum = sum + mesh_sum[((size_t)c * n_pair + p) * n_mesh + m];
            if (c < n_cols) flow_out[(size_t)c * n_pair + p] = sum;
            else area_out[p] = st->pair_g[(size_t)p] > 0.0 ? sum / st->pair_g[(size_t)p] : 0.0;
        }
    return PADNE_OK;
}
