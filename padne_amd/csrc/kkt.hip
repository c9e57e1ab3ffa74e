// solve_system on the device (solver.py:767-780 with everything around the solve call): the reference hands L and r to
// SuperLU and gets v back; here the KKT system is first reduced to an SPD one, and the bookkeeping of
// that reduction -- index map, right-hand side b = -P^T (r - L c), expansion v = c + P y, residual rows for the multiplier
// recovery, ||L v - r|| -- used to be numpy passes over N-element arrays plus three vector round trips over PCIe
// (0.10 s of a 0.14 s call at N = 10 M).  A padne_kkt plan keeps all of it on the device: the host describes the reduction
// by its O(#constraints) lists, r crosses PCIe once (while the reduced matrix and its multigrid hierarchy are being
// built), v once.
#include "common.hpp"
#include "error.hpp"                                  // GoalOut, csr_goal_error

#include <string.h>
#include <rocprim/device/device_radix_sort.hpp>      // the one stable key-value sort of the locality ordering (section "ordering")

#include <algorithm>
#include <cmath>
#include <math.h>
#include <string.h>
#include <thread>
#include <vector>

namespace padne {

int csr_relabel(padne_ctx *ctx, const padne_csr *m, const int32_t *row_map, int64_t n_rows_out, const int32_t *col_map,
                int64_t n_cols_out, double scale, padne_csr **out);
int amg_setup(padne_ctx *ctx, padne_csr *A0);
int csr_error_estimate(padne_ctx *ctx, const padne_csr *L, int **vptr, int **vface, int n_cols, const double *V_dev,
                       double *G_dev, double *eta_dev, double *mesh_E_dev, double *mesh_P_dev, double *mesh_max_dev,
                       long long *mesh_face_dev, int *bad_dev);
void amg_info(const padne_csr *A0, int *levels, double *complexity, double *setup_seconds, long long *coarse_n);

constexpr int kCopyStreams = 4;

}  // namespace padne

struct padne_kkt {
    padne_ctx *ctx = nullptr;
    const padne_csr *L = nullptr;        // borrowed: the caller keeps the assembled system alive
    long long N = 0, n_pot = 0, n_free = 0;
    int32_t *imap = nullptr;             // [N] reduced unknown of every unknown, -1 = none
    int32_t *src_of = nullptr;           // [n_free] the unknown whose row opens the sum of reduced row t (its representative)
    int32_t *tied_member = nullptr;      // [n_tied] further members of source-tied groups, ascending ...
    int32_t *tied_target = nullptr;      // [n_tied] ... and the reduced unknown they add into
    long long n_tied = 0;
    // the same list grouped by target (= by representative): entries tied_order[tied_gptr[g] .. tied_gptr[g + 1]) of the
    // two arrays above add into one reduced unknown, in ascending member order (kkt_rhs_tied: one thread per group)
    int32_t *tied_order = nullptr, *tied_gptr = nullptr;
    long long n_tied_groups = 0;
    padne_csr *A = nullptr;              // -P^T L P, owned (with its hierarchy once a solve has built it)
    // [N * vec_cap] device vectors: right-hand sides (the caller's layout), solutions, scratch, known parts (the products'
    // layout, see "blocks of right-hand sides")
    double *r = nullptr, *v = nullptr, *w = nullptr, *c = nullptr;
    double *b = nullptr, *y = nullptr;   // [(n_cols + n_extra) * n_free]
    double *Z = nullptr;                 // [n_extra * N] expanded extra solutions (regulators)
    long long vec_cap = 1;               // doubles per unknown the four N-vectors hold
    int rhs_cap = 1, z_cap = 0;          // reduced columns b and y hold, expanded extra solutions Z holds
    int n_cols = 1, n_extra = 0;         // of the last solve
    bool has_c = false, solved = false;
    // "finished": the last padne_kkt_finish_block left its final V on the device, [N][finished_cols] row-major in v_final (v,
    // or c when the products' layout differs from the caller's); any later solve clears it
    bool finished = false;
    const double *v_final = nullptr;
    int finished_cols = 0;
    // the block padne_kkt_combine_block formed, [N][finished_cols] (v_final points at it until the next solve frees it)
    double *combined = nullptr;
    double setup_seconds_last = 0.0;
    // vertex -> incident faces of L's mesh, rows in ascending face order (error.hip): built by the first
    // padne_kkt_error_estimate and kept, [mesh_n_vert + 1] and [3 mesh_n_tri]
    int *err_vptr = nullptr, *err_vface = nullptr;
};

namespace padne {

// ---- index map from the sparse description -----------------------------------------------------------------------
// imap[i] = i - #{e in elim : e < i} for potentials that are not eliminated, -1 otherwise (elim sorted, in LDS when short)
__global__ __launch_bounds__(256) void kkt_build_imap(const long long N, const long long n_pot, const long long *__restrict__ elim,
                                                      const int n_elim, int32_t *__restrict__ imap) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    if (i >= n_pot) {
        imap[i] = -1;
        return;
    }
    int lo = 0, hi = n_elim;                  // first position with elim[pos] >= i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (elim[mid] < i) lo = mid + 1; else hi = mid;
    }
    imap[i] = (lo < n_elim && elim[lo] == i) ? -1 : (int32_t)(i - lo);
}

__global__ void kkt_tie_members(const int n_tied, const long long *__restrict__ member, const long long *__restrict__ rep,
                                int32_t *__restrict__ imap, int32_t *__restrict__ tied_member, int32_t *__restrict__ tied_target) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_tied) return;
    const int32_t t = imap[rep[k]];           // representatives are never members themselves: their entry is final
    imap[member[k]] = t;
    tied_member[k] = (int32_t)member[k];
    tied_target[k] = t;
}

// src_of[imap[i]] = i; tied members may race with their representative for a slot -- kkt_fix_sources settles it afterwards
__global__ __launch_bounds__(256) void kkt_sources(const long long N, const int32_t *__restrict__ imap, int32_t *__restrict__ src_of) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int32_t t = imap[i];
    if (t >= 0) src_of[t] = (int32_t)i;
}

__global__ void kkt_fix_sources(const int n_tied, const long long *__restrict__ rep, const int32_t *__restrict__ imap,
                                int32_t *__restrict__ src_of) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_tied) src_of[imap[rep[k]]] = (int32_t)rep[k];
}

// ---- blocks of right-hand sides ------------------------------------------------------------------------------------
// A block of n_cols right-hand sides crosses PCIe in the caller's layout, [N][n_cols] row-major (r and the result).  The
// products with L read another one: columns in groups of 8, group g at offset 8 g N, laid out [N][w] with w the SpMM width of
// the group (8 for a full group; a last group of `count` columns is widened to 1, 2, 4 or 8, its spare columns zero).  For
// n_cols = 1, 2, 4 and 8 the two layouts coincide.  The elementwise stages read the caller's layout and write the products'
// one (or back), so no pass of its own converts between them; with n_cols = 1 every kernel below does exactly the
// arithmetic of the single-vector stage it generalises.
__host__ __device__ inline int kkt_group_width(int count) { return count >= 5 ? 8 : count >= 3 ? 4 : count; }

// entry (i, column j) in the products' layout
__host__ __device__ inline long long kkt_gidx(const long long N, const int n_cols, const int j, const long long i) {
    const int g = j >> 3;
    const int rest = n_cols - (g << 3);
    return (long long)g * 8 * N + i * kkt_group_width(rest < 8 ? rest : 8) + (j & 7);
}

// doubles per row of the products' layout
static inline long long kkt_block_width(int n_cols) {
    return 8LL * (n_cols / 8) + (n_cols % 8 != 0 ? kkt_group_width(n_cols % 8) : 0);
}

// dst[idx[p]] (column j, products' layout) = val[j][p], and the same into dst_caller ([N][n_cols]) if given
__global__ __launch_bounds__(256) void kkt_scatter_block(const int n, const long long N, const int n_cols, const long long *__restrict__ idx,
                                                         const double *__restrict__ val, double *__restrict__ dst,
                                                         double *__restrict__ dst_caller) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (p >= n) return;
    const long long i = idx[p];
    const double x = val[(long long)j * n + p];
    dst[kkt_gidx(N, n_cols, j, i)] = x;
    if (dst_caller != nullptr) dst_caller[i * n_cols + j] = x;
}

// r[row[e]][col[e]] = val[e] ([N][n_cols], zeroed before): a block of right-hand sides given by its non-zero entries
__global__ __launch_bounds__(256) void kkt_scatter_coo(const long long n, const int n_cols, const long long *__restrict__ row,
                                                       const int32_t *__restrict__ col, const double *__restrict__ val,
                                                       double *__restrict__ r) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256)
        r[row[e] * n_cols + col[e]] = val[e];
}

// ---- right-hand side: b = -P^T (r - L c) ---------------------------------------------------------------------------
// b[j][t] = -(r - Lc)[src_of[t], j] for every column j; the other members of a tied group are added by kkt_rhs_tied
__global__ __launch_bounds__(256) void kkt_rhs(const long long n_free, const long long N, const int n_cols, const int32_t *__restrict__ src_of,
                                               const double *__restrict__ r, const double *__restrict__ Lc, double *__restrict__ b) {
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n_free; t += (long long)gridDim.x * 256) {
        const long long i = src_of[t];
        for (int j = 0; j < n_cols; ++j) {
            const double ri = r[i * n_cols + j];
            b[(long long)j * n_free + t] = -(Lc != nullptr ? ri - Lc[kkt_gidx(N, n_cols, j, i)] : ri);
        }
    }
}

// One thread per tied GROUP (all further members of one representative) and column (blockIdx.y): it subtracts its members'
// terms from the group's reduced row one after the other in ascending member order -- the additions of a single thread
// walking the whole list in index order (what this kernel was: 0.2 s for 1e5 tied members, a chain of dependent
// read-modify-writes), in the same order per row, hence the same bits, in parallel over the rows.
__global__ __launch_bounds__(256) void kkt_rhs_tied(const int n_groups, const long long n_free, const long long N, const int n_cols,
                                                    const int32_t *__restrict__ gptr, const int32_t *__restrict__ order,
                                                    const int32_t *__restrict__ member, const int32_t *__restrict__ target,
                                                    const double *__restrict__ r, const double *__restrict__ Lc, double *__restrict__ b) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (g >= n_groups) return;
    const int e0 = gptr[g], e1 = gptr[g + 1];
    double *bj = b + (long long)j * n_free;
    const int32_t t = target[order[e0]];
    double acc = bj[t];
    for (int e = e0; e < e1; ++e) {
        const long long i = member[order[e]];
        const double ri = r[i * n_cols + j];
        acc -= (Lc != nullptr ? ri - Lc[kkt_gidx(N, n_cols, j, i)] : ri);
    }
    bj[t] = acc;
}

// extra right-hand sides (regulator gain columns): b_k = P^T gamma_k, a handful of entries each, added in list order
__global__ void kkt_rhs_extra(const int n_extra, const long long *__restrict__ ptr, const long long *__restrict__ row,
                              const double *__restrict__ val, const int32_t *__restrict__ imap, const long long n_free,
                              double *__restrict__ b_extra) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < n_extra; ++k)
        for (long long e = ptr[k]; e < ptr[k + 1]; ++e) {
            const int32_t t = imap[row[e]];
            if (t >= 0) b_extra[(long long)k * n_free + t] += val[e];
        }
}

// per-workgroup partial sums of a.a for up to 8 vectors laid out one after the other (stride n)
__global__ __launch_bounds__(256) void kkt_norm2(const long long n, const double *__restrict__ a, double *__restrict__ partials) {
    __shared__ double red[4];
    const double *v = a + (long long)blockIdx.y * n;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += v[i] * v[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long long)blockIdx.y * kMaxPartials + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[j] = sum of partials[j][0..P) in a fixed order (one workgroup per vector)
__global__ __launch_bounds__(256) void kkt_fold(const double *__restrict__ partials, const int P, double *__restrict__ out) {
    __shared__ double red[4];
    const double *p = partials + (long long)blockIdx.x * kMaxPartials;
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- expansion: v = c + P y (multipliers zero), every column (c, v in the products' layout; y: [n_cols][n_free]) ------
__global__ __launch_bounds__(256) void kkt_expand(const long long N, const int n_cols, const int32_t *__restrict__ imap,
                                                  const double *__restrict__ y, const long long n_free, const double *__restrict__ c,
                                                  double *__restrict__ v) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const int32_t t = imap[i];
        for (int j = 0; j < n_cols; ++j) {
            const long long g = kkt_gidx(N, n_cols, j, i);
            const double known = c != nullptr ? c[g] : 0.0;
            v[g] = t >= 0 ? known + y[(long long)j * n_free + t] : known;
        }
    }
}

// out[j][p] = (r - L v)[idx[p], j]: the KCL residual rows of the multiplier recovery, at the probed unknowns only
__global__ __launch_bounds__(256) void kkt_rho_probe(const int n_probe, const long long N, const int n_cols, const long long *__restrict__ idx,
                                                     const double *__restrict__ r, const double *__restrict__ Lv, double *__restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (p >= n_probe) return;
    const long long i = idx[p];
    out[(long long)j * n_probe + p] = r[i * n_cols + j] - Lv[kkt_gidx(N, n_cols, j, i)];
}

__global__ void kkt_gather_f64(const int n, const long long *__restrict__ idx, const double *__restrict__ src, double *__restrict__ dst) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = src[idx[k]];
}

// v[:, j] += sum_k coeff[j][k] Z_k for every column j (Z_k shared by all columns), and the result also into v_caller
// ([N][n_cols]) if given
__global__ __launch_bounds__(256) void kkt_add_extras(const long long N, const int n_cols, const int n_extra, const double *__restrict__ coeff,
                                                      const double *__restrict__ Z, double *__restrict__ v, double *__restrict__ v_caller) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        for (int j = 0; j < n_cols; ++j) {
            const long long g = kkt_gidx(N, n_cols, j, i);
            double s = v[g];
            for (int k = 0; k < n_extra; ++k) s += coeff[(long long)j * n_extra + k] * Z[(long long)k * N + i];
            v[g] = s;
            if (v_caller != nullptr) v_caller[i * n_cols + j] = s;
        }
    }
}

// per-workgroup partial sums of (Lv - r)^2 of column blockIdx.y (Lv in the products' layout, r in the caller's)
__global__ __launch_bounds__(256) void kkt_diff2(const long long N, const int n_cols, const double *__restrict__ Lv,
                                                 const double *__restrict__ r, double *__restrict__ partials) {
    __shared__ double red[4];
    const int j = blockIdx.y;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const double d = Lv[kkt_gidx(N, n_cols, j, i)] - r[i * n_cols + j];
        s += d * d;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long long)j * kMaxPartials + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- locality ordering of the reduced unknowns ("Ordering") ----------------------------------------
// CGAL numbers vertices in insertion order; the reduced system is solved in a band numbering by horizontal strips: the mesh
// unknowns sorted by (mesh, strip of about three vertex spacings, x), the others behind them in their old order.  The host
// form (reduction.apply_locality_ordering: numpy sorts over N-element arrays) was 0.09 s of a 0.14 s solve_system call on a
// 2 M-vertex mesh; here the keys are formed and sorted on the device from the mesh the system was assembled from.  Per-mesh
// constants (bounding box of the owners, strip height) come from a small reduction and the host's own formula, so that
// the keys -- and with a stable sort the permutation -- are the host's bit for bit (tested).
// stats[m] = {x min, x max, y min, y max, count} over the mesh vertices that represent a reduced unknown
__global__ __launch_bounds__(256) void kkt_mesh_stats(const long long *__restrict__ voff, const double *__restrict__ xy,
                                                      const int32_t *__restrict__ imap, const int32_t *__restrict__ src_of,
                                                      double *__restrict__ stats) {
    __shared__ double red[5][4];
    const int m = blockIdx.x;
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300, cnt = 0.0;
    for (long long v = voff[m] + threadIdx.x; v < voff[m + 1]; v += 256) {
        const int32_t t = imap[v];
        if (t < 0 || src_of[t] != (int32_t)v) continue;
        const double x = xy[2 * v], y = xy[2 * v + 1];
        xmin = fmin(xmin, x);
        xmax = fmax(xmax, x);
        ymin = fmin(ymin, y);
        ymax = fmax(ymax, y);
        cnt += 1.0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        xmin = fmin(xmin, __shfl_down(xmin, off, 64));
        xmax = fmax(xmax, __shfl_down(xmax, off, 64));
        ymin = fmin(ymin, __shfl_down(ymin, off, 64));
        ymax = fmax(ymax, __shfl_down(ymax, off, 64));
        cnt += __shfl_down(cnt, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = xmin; red[1][w] = xmax; red[2][w] = ymin; red[3][w] = ymax; red[4][w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[5 * m + 0] = fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3]));
        stats[5 * m + 1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
        stats[5 * m + 2] = fmin(fmin(red[2][0], red[2][1]), fmin(red[2][2], red[2][3]));
        stats[5 * m + 3] = fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3]));
        stats[5 * m + 4] = (red[4][0] + red[4][1]) + (red[4][2] + red[4][3]);
    }
}

// key[t] = mesh << (32 + strip_bits) | strip << 32 | x quantised to 32 bits inside the mesh; unknowns that are no mesh
// vertex: n_mesh in the mesh field | t.  The same ORDER as the host's keys [mesh 16 | strip 16 | x 32] with 0xFFFF for the
// unknowns behind the vertices -- every field keeps its rank -- in as few bits as the system needs, so that the radix
// sort behind it walks 40-odd bits instead of 64.
// par[m] = {x lo, x span, y0, strip height} as the host computes them (reduction._strip_order / strip_index)
__global__ __launch_bounds__(256) void kkt_strip_keys(const long long n_free, const long long n_vert, const int n_mesh,
                                                      const long long *__restrict__ voff, const double *__restrict__ xy,
                                                      const int32_t *__restrict__ src_of, const double *__restrict__ par,
                                                      unsigned long long *__restrict__ key, int *__restrict__ val, int *__restrict__ bad,
                                                      const int strip_bits) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_free) return;
    val[t] = (int)t;
    const long long v = src_of[t];
    if (v >= n_vert) {
        key[t] = ((unsigned long long)n_mesh << (32 + strip_bits)) | (unsigned long long)t;
        return;
    }
    int lo = 0, hi = n_mesh;                       // mesh of v: largest m with voff[m] <= v
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (voff[mid] <= v) lo = mid; else hi = mid;
    }
    const int m = lo;
    const double x = xy[2 * v], y = xy[2 * v + 1];
    const double x_lo = par[4 * m], span = par[4 * m + 1], y0 = par[4 * m + 2], height = par[4 * m + 3];
    long long strip = 0;
    if (height > 0.0) strip = (long long)fmin(floor((y - y0) / height), 65536.0);      // (clamped before the cast, as the host's)
    if (strip < 0 || strip >= (1ll << strip_bits)) {        // (the host's bound of the field, computed from the same numbers)
        atomicExch(bad, 1);
        strip = 0;
    }
    double q = (x - x_lo) / span * 4294967295.0;
    if (q > 4294967295.0) q = 4294967295.0;
    const unsigned long long xq = (unsigned long long)q;
    key[t] = ((unsigned long long)m << (32 + strip_bits)) | ((unsigned long long)strip << 32) | xq;
}

__global__ void kkt_invert_perm(const long long n, const int *__restrict__ order, int32_t *__restrict__ new_of_old) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) new_of_old[order[k]] = (int32_t)k;
}

__global__ void kkt_relabel_map(const long long N, const int32_t *__restrict__ new_of_old, int32_t *__restrict__ imap) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t t = imap[i];
    if (t >= 0) imap[i] = new_of_old[t];
}

__global__ void kkt_permute_i32(const long long n, const int *__restrict__ order, const int32_t *__restrict__ src, int32_t *__restrict__ dst) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = src[order[k]];
}

__global__ void kkt_relabel_list(const int n, const int32_t *__restrict__ new_of_old, int32_t *__restrict__ list) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) list[k] = new_of_old[list[k]];
}

// relabels k->imap / src_of / tied_target in place; PADNE_E_INVALID (nothing changed) when the keys do not fit their fields
static int kkt_apply_strip_order(padne_kkt *k) {
    padne_ctx *ctx = k->ctx;
    const padne_csr *L = k->L;
    hipStream_t s = ctx->stream;
    const long long nf = k->n_free, nv = L->mesh_n_vert;
    const int n_mesh = (int)L->mesh_n_mesh;
    if (nf == 0) return PADNE_OK;
    PADNE_REQUIRE(n_mesh > 0 && L->mesh_xy != nullptr && L->mesh_voff != nullptr, "the system matrix carries no mesh to order by");
    PADNE_REQUIRE(n_mesh < 0xFFFF && nf < 2147483647LL && nv <= k->n_pot, "mesh count / size beyond the key fields");
    Scratch sc(ctx);
    double *d_stats = nullptr, *d_par = nullptr;
    unsigned long long *key_a = nullptr, *key_b = nullptr;
    int *val_a = nullptr, *val_b = nullptr, *d_bad = nullptr;
    int32_t *new_of_old = nullptr, *src_new = nullptr;
    PADNE_TRY(sc.alloc(&d_stats, (size_t)5 * n_mesh));
    PADNE_TRY(sc.alloc(&d_par, (size_t)4 * n_mesh));
    PADNE_TRY(sc.alloc(&key_a, (size_t)nf));
    PADNE_TRY(sc.alloc(&key_b, (size_t)nf));
    PADNE_TRY(sc.alloc(&val_a, (size_t)nf));
    PADNE_TRY(sc.alloc(&val_b, (size_t)nf));
    PADNE_TRY(sc.alloc(&d_bad, 1));
    PADNE_TRY(sc.alloc(&new_of_old, (size_t)nf));
    PADNE_TRY(sc.alloc(&src_new, (size_t)nf));
    hipLaunchKernelGGL(kkt_mesh_stats, dim3(n_mesh), dim3(256), 0, s, L->mesh_voff, L->mesh_xy, k->imap, k->src_of, d_stats);
    PADNE_HIP_CHECK(hipGetLastError());
    std::vector<double> st((size_t)5 * n_mesh), par((size_t)4 * n_mesh);
    PADNE_HIP_CHECK(hipMemcpyAsync(st.data(), d_stats, sizeof(double) * st.size(), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    double strips_max = 1.0;                                // largest strip index any mesh can produce (+ 1 of slack for the rounding of floor)
    for (int m = 0; m < n_mesh; ++m) {
        const double xmin = st[5 * m], xmax = st[5 * m + 1], ymin = st[5 * m + 2], ymax = st[5 * m + 3], cnt = st[5 * m + 4];
        double x_lo = 0.0, span = 1.0, y0 = 0.0, height = 0.0;
        if (cnt >= 1.0) {
            x_lo = xmin;
            span = std::max(xmax - xmin, 1e-300);                               // reduction._strip_order
            y0 = ymin;
            // reduction.strip_index (a single point: strip 0).  A box of the owners with zero width or zero height has no area
            // to take a spacing from: height stays 0 and kkt_strip_keys gives every owner of the mesh strip 0, the host's rule
            if (cnt >= 2.0 && xmax - xmin != 0.0 && ymax - y0 != 0.0) {
                const double area = std::max((xmax - xmin) * (ymax - y0), 1e-300);
                height = 3.4 * sqrt(area / cnt);
            }
        }
        if (height > 0.0) strips_max = std::max(strips_max, floor((ymax - y0) / height) + 2.0);
        par[4 * m] = x_lo;
        par[4 * m + 1] = span;
        par[4 * m + 2] = y0;
        par[4 * m + 3] = height;
    }
    PADNE_HIP_CHECK(hipMemcpyAsync(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, s));
    PADNE_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    // the fields of the sort key, as narrow as this system allows: strips (at most 16 bits, the host's field), meshes + 1
    int strip_bits = 1, mesh_bits = 1;
    while (strip_bits < 16 && (double)(1ll << strip_bits) <= strips_max) ++strip_bits;
    while ((1ll << mesh_bits) <= (long long)n_mesh) ++mesh_bits;
    const int key_bits = 32 + strip_bits + mesh_bits;      // <= 32 + 16 + 16
    hipLaunchKernelGGL(kkt_strip_keys, dim3(nblk(nf)), dim3(256), 0, s, nf, nv, n_mesh, L->mesh_voff, L->mesh_xy, k->src_of, d_par,
                       key_a, val_a, d_bad, strip_bits);
    PADNE_HIP_CHECK(hipGetLastError());
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));              // (also: par's host buffer may go)
    if (h_bad) {
        set_error("strip index beyond 16 bits: the host orders this system");
        return PADNE_E_INVALID;
    }
    // stable sort of (key, old index): equal keys keep their index order, as the host's tie repair leaves them
    size_t tmp_bytes = 0;
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_a, key_b, val_a, val_b, (size_t)nf, 0, key_bits, s));
    void *tmp = nullptr;
    PADNE_TRY(sc.alloc((char **)&tmp, tmp_bytes));
    PADNE_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, val_b, (size_t)nf, 0, key_bits, s));
    const int *order = val_b;                              // new position -> old reduced index
    hipLaunchKernelGGL(kkt_invert_perm, dim3(nblk(nf)), dim3(256), 0, s, nf, order, new_of_old);
    hipLaunchKernelGGL(kkt_relabel_map, dim3(nblk(k->N)), dim3(256), 0, s, k->N, (const int32_t *)new_of_old, k->imap);
    hipLaunchKernelGGL(kkt_permute_i32, dim3(nblk(nf)), dim3(256), 0, s, nf, order, (const int32_t *)k->src_of, src_new);
    if (k->n_tied > 0)
        hipLaunchKernelGGL(kkt_relabel_list, dim3(nblk(k->n_tied)), dim3(256), 0, s, (int)k->n_tied, (const int32_t *)new_of_old,
                           k->tied_target);
    PADNE_HIP_CHECK(hipGetLastError());
    PADNE_HIP_CHECK(hipMemcpyAsync(k->src_of, src_new, sizeof(int32_t) * (size_t)nf, hipMemcpyDeviceToDevice, s));
    return PADNE_OK;
}

static int vgrid(long long n) {
    long long g = (n + 255) / 256;
    if (g > 1024) g = 1024;
    return (int)(g < 1 ? 1 : g);
}

// A pageable host buffer crosses PCIe through the runtime's pinned staging area at the speed of ONE host core's memcpy
// (8-10 GB/s: 8-10 ms for the 80 MB of a 10 M-unknown vector); kCopyStreams threads, each with a stream and a quarter
// of the vector, bring it close to the link.  Blocks the caller until all parts have arrived.
static int copy_streams(padne_ctx *ctx, int count) {      // the context's first `count` copy streams exist
    static_assert(kCopyStreams == sizeof(ctx->copy_stream) / sizeof(ctx->copy_stream[0]), "the context holds the copy streams");
    for (int t = 0; t < count; ++t)
        if (ctx->copy_stream[t] == nullptr && hipStreamCreateWithFlags(&ctx->copy_stream[t], hipStreamNonBlocking) != hipSuccess) {
            ctx->copy_stream[t] = nullptr;
            set_error("stream creation failed");
            return PADNE_E_HIP;
        }
    return PADNE_OK;
}

static int parallel_copy(padne_kkt *k, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    const int device = k->ctx->device;
    hipStream_t *copy_stream = k->ctx->copy_stream;
    if (bytes < ((size_t)8 << 20)) {
        PADNE_TRY(copy_streams(k->ctx, 1));
        PADNE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, copy_stream[0]));
        PADNE_HIP_CHECK(hipStreamSynchronize(copy_stream[0]));
        return PADNE_OK;
    }
    PADNE_TRY(copy_streams(k->ctx, kCopyStreams));
    hipError_t err[kCopyStreams];
    std::thread th[kCopyStreams];
    const size_t chunk = ((bytes / kCopyStreams) + 4095) & ~(size_t)4095;
    for (int t = 0; t < kCopyStreams; ++t) {
        const size_t off = std::min(bytes, (size_t)t * chunk), len = std::min(bytes - off, chunk);
        err[t] = hipSuccess;
        th[t] = std::thread([=, &err]() {
            if (len == 0) return;
            hipError_t e = hipSetDevice(device);
            if (e == hipSuccess) e = hipMemcpyAsync((char *)dst + off, (const char *)src + off, len, kind, copy_stream[t]);
            if (e == hipSuccess) e = hipStreamSynchronize(copy_stream[t]);
            err[t] = e;
        });
    }
    for (int t = 0; t < kCopyStreams; ++t) th[t].join();
    for (int t = 0; t < kCopyStreams; ++t)
        if (err[t] != hipSuccess) {
            set_error("vector transfer failed: %s", hipGetErrorString(err[t]));
            return PADNE_E_HIP;
        }
    return PADNE_OK;
}

static void kkt_free(padne_kkt *k) {
    if (k == nullptr) return;
    padne_ctx *ctx = k->ctx;
    if (ctx != nullptr && ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
    if (ctx != nullptr)
        for (hipStream_t cs : ctx->copy_stream)
            if (cs != nullptr) (void)hipStreamSynchronize(cs);
    if (k->A != nullptr) padne_csr_destroy(k->A);
    for (void *p : {(void *)k->imap, (void *)k->src_of, (void *)k->tied_member, (void *)k->tied_target, (void *)k->tied_order,
                    (void *)k->tied_gptr, (void *)k->r, (void *)k->v,
                    (void *)k->w, (void *)k->c, (void *)k->b, (void *)k->y, (void *)k->Z, (void *)k->err_vptr,
                    (void *)k->err_vface, (void *)k->combined})
        if (p != nullptr) pool_free(ctx, p);
    delete k;
}

}  // namespace padne

using namespace padne;

extern "C" int padne_kkt_create(padne_ctx *ctx, const padne_csr *L, int64_t n_potential, int64_t n_elim,
                                const int64_t *elim_sorted, int64_t n_tied, const int64_t *tied_member,
                                const int64_t *tied_rep, const int32_t *index_map_host, int64_t n_free, int32_t flags,
                                padne_kkt **out) {
    PADNE_REQUIRE(ctx && L && out, "null argument");
    PADNE_REQUIRE(L->n_rows == L->n_cols, "the system matrix must be square");
    const long long N = L->n_rows;
    PADNE_REQUIRE(n_potential >= 0 && n_potential <= N, "n_potential");
    PADNE_REQUIRE(n_elim >= 0 && n_tied >= 0 && n_tied <= n_elim && n_elim < 2147483647LL, "list sizes");
    PADNE_REQUIRE(n_elim == 0 || elim_sorted != nullptr, "elim list");
    PADNE_REQUIRE(n_tied == 0 || (tied_member != nullptr && tied_rep != nullptr), "tied lists");
    PADNE_REQUIRE(n_free >= 0 && n_free <= n_potential, "n_free");
    PADNE_REQUIRE(index_map_host != nullptr || n_free == n_potential - n_elim, "n_free does not match the lists");
    for (int64_t k = 0; k < n_elim; ++k)
        PADNE_REQUIRE(elim_sorted[k] >= 0 && elim_sorted[k] < n_potential && (k == 0 || elim_sorted[k - 1] < elim_sorted[k]),
                      "elim list must be sorted, unique and inside the potentials");
    for (int64_t k = 0; k < n_tied; ++k) {
        PADNE_REQUIRE(tied_member[k] >= 0 && tied_member[k] < n_potential && tied_rep[k] >= 0 && tied_rep[k] < n_potential &&
                      tied_rep[k] != tied_member[k] && (k == 0 || tied_member[k - 1] < tied_member[k]),
                      "tied lists must be sorted by member and inside the potentials");
        PADNE_REQUIRE(std::binary_search(elim_sorted, elim_sorted + n_elim, tied_member[k]) &&
                      !std::binary_search(elim_sorted, elim_sorted + n_elim, tied_rep[k]),
                      "a tied member must be eliminated and its representative must not be");
    }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_kkt *k = new padne_kkt();
    k->ctx = ctx;
    k->L = L;
    k->N = N;
    k->n_pot = n_potential;
    k->n_free = n_free;
    k->n_tied = n_tied;
    int rc = PADNE_OK;
    auto fail = [&](int code) {
        kkt_free(k);
        return code;
    };
    // (the copy streams of the context, made here on the calling thread: the copies themselves run on threads of their own)
    if (copy_streams(ctx, sizeof(double) * (size_t)(N > 0 ? N : 1) >= ((size_t)8 << 20) ? kCopyStreams : 1) != PADNE_OK) return fail(PADNE_E_HIP);
    const size_t nN = (size_t)(N > 0 ? N : 1), nF = (size_t)(n_free > 0 ? n_free : 1), nT = (size_t)(n_tied > 0 ? n_tied : 1);
    k->imap = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * nN);
    k->src_of = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * nF);
    k->tied_member = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * nT);
    k->tied_target = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * nT);
    k->r = (double *)pool_alloc(ctx, sizeof(double) * nN);
    k->v = (double *)pool_alloc(ctx, sizeof(double) * nN);
    k->w = (double *)pool_alloc(ctx, sizeof(double) * nN);
    k->c = (double *)pool_alloc(ctx, sizeof(double) * nN);
    k->b = (double *)pool_alloc(ctx, sizeof(double) * nF);
    k->y = (double *)pool_alloc(ctx, sizeof(double) * nF);
    if (!k->imap || !k->src_of || !k->tied_member || !k->tied_target || !k->r || !k->v || !k->w || !k->c || !k->b || !k->y)
        return fail(PADNE_E_NOMEM);
    Scratch sc(ctx);
    long long *d_elim = nullptr, *d_mem = nullptr, *d_rep = nullptr;
    if ((rc = sc.alloc(&d_elim, (size_t)n_elim)) != PADNE_OK || (rc = sc.alloc(&d_mem, (size_t)n_tied)) != PADNE_OK ||
        (rc = sc.alloc(&d_rep, (size_t)n_tied)) != PADNE_OK)
        return fail(rc);
    hipError_t e = hipSuccess;
    std::vector<int32_t> h_order, h_gptr;                  // (outlive the asynchronous copies below: synchronised before return)
    if (n_tied > 0) {
        e = hipMemcpyAsync(d_mem, tied_member, sizeof(long long) * (size_t)n_tied, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_rep, tied_rep, sizeof(long long) * (size_t)n_tied, hipMemcpyHostToDevice, s);
        // the list grouped by representative; inside a group the members keep their (ascending) order
        h_order.resize((size_t)n_tied);
        for (int64_t q = 0; q < n_tied; ++q) h_order[(size_t)q] = (int32_t)q;
        std::stable_sort(h_order.begin(), h_order.end(), [&](int32_t a, int32_t b) { return tied_rep[a] < tied_rep[b]; });
        for (int64_t q = 0; q < n_tied; ++q)
            if (q == 0 || tied_rep[h_order[(size_t)q]] != tied_rep[h_order[(size_t)q - 1]]) h_gptr.push_back((int32_t)q);
        k->n_tied_groups = (long long)h_gptr.size();
        h_gptr.push_back((int32_t)n_tied);
        k->tied_order = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * h_order.size());
        k->tied_gptr = (int32_t *)pool_alloc(ctx, sizeof(int32_t) * h_gptr.size());
        if (!k->tied_order || !k->tied_gptr) return fail(PADNE_E_NOMEM);
        if (e == hipSuccess) e = hipMemcpyAsync(k->tied_order, h_order.data(), sizeof(int32_t) * h_order.size(), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(k->tied_gptr, h_gptr.data(), sizeof(int32_t) * h_gptr.size(), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess && index_map_host != nullptr) {
        // a map the host made (locality reordering of a scattered numbering): used as it is
        e = hipMemcpyAsync(k->imap, index_map_host, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && n_tied > 0) {
            // tied_target straight from the uploaded map
            hipLaunchKernelGGL(kkt_tie_members, dim3(nblk(n_tied)), dim3(256), 0, s, (int)n_tied, d_mem, d_mem, k->imap,
                               k->tied_member, k->tied_target);
            e = hipGetLastError();
        }
    } else if (e == hipSuccess) {
        if (n_elim > 0) e = hipMemcpyAsync(d_elim, elim_sorted, sizeof(long long) * (size_t)n_elim, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && N > 0) {
            hipLaunchKernelGGL(kkt_build_imap, dim3(nblk(N)), dim3(256), 0, s, N, (long long)n_potential, d_elim, (int)n_elim, k->imap);
            if (n_tied > 0)
                hipLaunchKernelGGL(kkt_tie_members, dim3(nblk(n_tied)), dim3(256), 0, s, (int)n_tied, d_mem, d_rep, k->imap,
                                   k->tied_member, k->tied_target);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && N > 0) {
        hipLaunchKernelGGL(kkt_sources, dim3(nblk(N)), dim3(256), 0, s, N, k->imap, k->src_of);
        if (n_tied > 0)
            hipLaunchKernelGGL(kkt_fix_sources, dim3(nblk(n_tied)), dim3(256), 0, s, (int)n_tied, d_rep, k->imap, k->src_of);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        set_error("building the index map failed: %s", hipGetErrorString(e));
        return fail(PADNE_E_HIP);
    }
    if ((flags & 1) != 0 && index_map_host == nullptr) {
        // the reduced unknowns in the strip numbering (mesh, strip, x) of the mesh the system was assembled from
        if ((rc = kkt_apply_strip_order(k)) != PADNE_OK) return fail(rc);
    }
    // A = -P^T L P from the device-resident map (csr_relabel takes host or device maps)
    if ((rc = csr_relabel(ctx, L, k->imap, n_free, k->imap, n_free, -1.0, &k->A)) != PADNE_OK) return fail(rc);
    if (hipStreamSynchronize(s) != hipSuccess) {      // the scratch lists go out of scope
        set_error("plan creation failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(PADNE_E_HIP);
    }
    *out = k;
    return PADNE_OK;
}

extern "C" int padne_kkt_destroy(padne_kkt *k) {
    if (k != nullptr && k->ctx != nullptr) (void)hipSetDevice(k->ctx->device);
    kkt_free(k);
    return PADNE_OK;
}

extern "C" int padne_kkt_matrix(const padne_kkt *k, const padne_csr **reduced_out) {
    PADNE_REQUIRE(k && reduced_out, "null argument");
    *reduced_out = k->A;
    return PADNE_OK;
}

// y = L x for n_cols vectors in the products' layout: one pass over L per group of up to 8 columns (SpMM of width 8 / 4 / 2,
// a single column SpMV -- for n_cols = 1 the product of the vector path)
static int kkt_products(padne_ctx *ctx, const padne_kkt *k, const int n_cols, const double *x, double *y) {
    for (int first = 0; first < n_cols; first += 8) {
        const int w = kkt_group_width(std::min(8, n_cols - first));
        const long long off = (long long)first * k->N;
        if (w == 1) PADNE_TRY(launch_spmv(ctx, k->L, x + off, y + off, nullptr, nullptr, nullptr));
        else PADNE_TRY((launch_spmm<double, double>(ctx, k->L, w, SPMV_PLAIN, x + off, y + off, {})));
    }
    return PADNE_OK;
}

// The right-hand sides of a stage 1: a dense block r_host[N][n_cols], the same block already on the device (dense_dev), or
// (both null) n_entries COO triples
struct KktRhs {
    const double *dense = nullptr;
    const double *dense_dev = nullptr;
    int64_t n_entries = 0;
    const int64_t *row = nullptr;
    const int32_t *col = nullptr;
    const double *val = nullptr;
};

// Stage 1 for a block of n_cols right-hand sides (n_cols = 1: padne_kkt_solve)
static int kkt_solve_block(padne_ctx *ctx, padne_kkt *k, const int n_cols, const KktRhs &rhs, int64_t n_known,
                           const int64_t *known_idx, const double *known_val, int32_t n_extra, const int64_t *extra_ptr,
                           const int64_t *extra_row, const double *extra_val, int64_t n_probe, const int64_t *probe_idx,
                           double *probe_out, const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info) {
    const double *r_host = rhs.dense;
    PADNE_REQUIRE(ctx && k && opts, "null argument");
    PADNE_REQUIRE(k->ctx == ctx, "the plan belongs to another context");
    k->finished = false;
    if (k->combined != nullptr) {            // a combined block ends with the solve that follows it
        pool_free(ctx, k->combined);
        k->combined = nullptr;
        k->v_final = nullptr;
    }
    PADNE_REQUIRE(r_host != nullptr || rhs.n_entries == 0 || (rhs.row && rhs.col && rhs.val), "null argument");
    PADNE_REQUIRE(n_cols >= 1 && n_extra >= 0 && n_cols + n_extra <= 4096, "at most 4096 right-hand sides with the extra ones");
    PADNE_REQUIRE(r_host != nullptr || rhs.n_entries >= 0, "number of right-hand side entries");
    if (r_host == nullptr && rhs.n_entries > 0) {
        // every (row, column) pair once and inside the block: the scatter below writes each entry of r at most once
        std::vector<long long> keys((size_t)rhs.n_entries);
        for (int64_t e = 0; e < rhs.n_entries; ++e) {
            PADNE_REQUIRE(rhs.row[e] >= 0 && rhs.row[e] < k->N && rhs.col[e] >= 0 && rhs.col[e] < n_cols,
                          "right-hand side entry out of range");
            keys[(size_t)e] = (long long)rhs.row[e] * n_cols + rhs.col[e];
        }
        std::sort(keys.begin(), keys.end());
        PADNE_REQUIRE(std::adjacent_find(keys.begin(), keys.end()) == keys.end(), "duplicate (row, column) pair in the right-hand sides");
    }
    PADNE_REQUIRE(n_known >= 0 && (n_known == 0 || (known_idx && known_val)), "known potentials");
    PADNE_REQUIRE(n_extra == 0 || (extra_ptr && extra_ptr[0] == 0), "extra right-hand sides");
    PADNE_REQUIRE(n_probe >= 0 && (n_probe == 0 || (probe_idx && probe_out)), "probes");
    const long long N = k->N, nf = k->n_free;
    for (int64_t j = 0; j < n_known; ++j) PADNE_REQUIRE(known_idx[j] >= 0 && known_idx[j] < k->n_pot, "known potential out of range");
    for (int64_t j = 0; j < n_probe; ++j) PADNE_REQUIRE(probe_idx[j] >= 0 && probe_idx[j] < N, "probe out of range");
    const long long n_ex_entries = n_extra > 0 ? extra_ptr[n_extra] : 0;
    for (int j = 0; j < n_extra; ++j) PADNE_REQUIRE(extra_ptr[j] <= extra_ptr[j + 1], "extra_ptr must be monotone");
    PADNE_REQUIRE(n_ex_entries == 0 || (extra_row && extra_val), "extra entries");
    for (long long e = 0; e < n_ex_entries; ++e) PADNE_REQUIRE(extra_row[e] >= 0 && extra_row[e] < N, "extra row out of range");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    padne_solve_info local;
    memset(&local, 0, sizeof(local));
    const int n_rhs = n_cols + n_extra;      // reduced columns: the block's, then the regulators' (solved once per block)
    local.n_rhs = n_rhs;
    k->solved = false;
    k->n_cols = n_cols;
    k->n_extra = n_extra;
    // a wider block or more right-hand sides than last time: grow the N-vectors, b and y, Z (none of them is in flight: the
    // copy streams were synchronised when their last transfer ended)
    const long long width = kkt_block_width(n_cols);
    const size_t nN = (size_t)(N > 0 ? N : 1), nF = (size_t)(nf > 0 ? nf : 1);
    if (width > k->vec_cap || n_rhs > k->rhs_cap || n_extra > k->z_cap) PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (width > k->vec_cap) {
        for (double **p : {&k->r, &k->v, &k->w, &k->c}) {
            pool_free(ctx, *p);
            *p = (double *)pool_alloc(ctx, sizeof(double) * nN * (size_t)width);
        }
        k->vec_cap = 0;
        if (!k->r || !k->v || !k->w || !k->c) return PADNE_E_NOMEM;
        k->vec_cap = width;
    }
    if (n_rhs > k->rhs_cap) {
        for (double **p : {&k->b, &k->y}) {
            pool_free(ctx, *p);
            *p = (double *)pool_alloc(ctx, sizeof(double) * nF * (size_t)n_rhs);
        }
        k->rhs_cap = 0;
        if (!k->b || !k->y) return PADNE_E_NOMEM;
        k->rhs_cap = n_rhs;
    }
    if (n_extra > k->z_cap) {
        pool_free(ctx, k->Z);
        k->Z = (double *)pool_alloc(ctx, sizeof(double) * nN * (size_t)n_extra);
        k->z_cap = 0;
        if (!k->Z) return PADNE_E_NOMEM;
        k->z_cap = n_extra;
    }
    // 1. R crosses PCIe on its own streams, in the caller's layout, while this thread builds what does not depend on it:
    //    1/diag, the x-window plan and the multigrid hierarchy of A (the counterpart of the factorisation)
    //    (a block given by its entries: r is zeroed and the entries scattered into it on the stream, ahead of that work)
    int up_rc = PADNE_OK;
    std::thread uploader;
    struct Join {
        std::thread &t;
        ~Join() { if (t.joinable()) t.join(); }
    } join_guard{uploader};
    Scratch sc_r(ctx);
    if (r_host != nullptr) {
        uploader = std::thread([&]() {
            (void)hipSetDevice(ctx->device);
            up_rc = parallel_copy(k, k->r, r_host, sizeof(double) * (size_t)N * (size_t)n_cols, hipMemcpyHostToDevice);
        });
    } else if (rhs.dense_dev != nullptr) {
        // a block another handle formed on the device: one copy on the stream into the plan's r, in the same layout
        PADNE_HIP_CHECK(hipMemcpyAsync(k->r, rhs.dense_dev, sizeof(double) * (size_t)N * (size_t)n_cols, hipMemcpyDeviceToDevice, s));
    } else {
        PADNE_HIP_CHECK(hipMemsetAsync(k->r, 0, sizeof(double) * (size_t)N * (size_t)n_cols, s));
        if (rhs.n_entries > 0) {
            long long *d_row = nullptr;
            int32_t *d_col = nullptr;
            double *d_val = nullptr;
            PADNE_TRY(sc_r.alloc(&d_row, (size_t)rhs.n_entries));
            PADNE_TRY(sc_r.alloc(&d_col, (size_t)rhs.n_entries));
            PADNE_TRY(sc_r.alloc(&d_val, (size_t)rhs.n_entries));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_row, rhs.row, sizeof(long long) * (size_t)rhs.n_entries, hipMemcpyHostToDevice, s));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_col, rhs.col, sizeof(int32_t) * (size_t)rhs.n_entries, hipMemcpyHostToDevice, s));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_val, rhs.val, sizeof(double) * (size_t)rhs.n_entries, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(kkt_scatter_coo, dim3(vgrid(rhs.n_entries)), dim3(256), 0, s, (long long)rhs.n_entries, n_cols, d_row,
                               d_col, d_val, k->r);
            PADNE_HIP_CHECK(hipGetLastError());
        }
    }
    if ((opts->flags & 4) != 0 && k->A->amg != nullptr) {
        amg_destroy(k->A->amg);
        k->A->amg = nullptr;
    }
    const bool want_amg = opts->precond == 1 && nf > kTinySystem;
    double setup_s = 0.0;
    if (nf > 0) {
        PADNE_TRY(csr_build_dinv(ctx, k->A));
        PADNE_TRY(csr_build_xw_plan(ctx, k->A));
        if (want_amg && k->A->amg == nullptr) {
            const int rc_setup = amg_setup(ctx, k->A);
            if (rc_setup != PADNE_OK && rc_setup != PADNE_E_NOCOARSEN) return rc_setup;
            if (rc_setup == PADNE_OK) amg_info(k->A, nullptr, nullptr, &setup_s, nullptr);
        }
    }
    k->setup_seconds_last = setup_s;
    auto products = [&](const double *x, double *y) { return kkt_products(ctx, k, n_cols, x, y); };
    // the spare columns of a widened last group: zero where the products read them
    const int last = n_cols - ((n_cols - 1) / 8) * 8, last_w = kkt_group_width(last);
    const long long last_off = (long long)((n_cols - 1) / 8) * 8 * N;
    // known part of the potentials: c (zero unless sources fix potentials against the ground or against each other)
    Scratch sc(ctx);
    k->has_c = n_known > 0;
    if (k->has_c) {
        long long *d_idx = nullptr;
        double *d_val = nullptr;
        PADNE_TRY(sc.alloc(&d_idx, (size_t)n_known));
        PADNE_TRY(sc.alloc(&d_val, (size_t)n_known * (size_t)n_cols));
        PADNE_HIP_CHECK(hipMemsetAsync(k->c, 0, sizeof(double) * (size_t)N * (size_t)width, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_idx, known_idx, sizeof(long long) * (size_t)n_known, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_val, known_val, sizeof(double) * (size_t)n_known * (size_t)n_cols, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(kkt_scatter_block, dim3(nblk(n_known), n_cols), dim3(256), 0, s, (int)n_known, N, n_cols, d_idx, d_val,
                           k->c, (double *)nullptr);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_TRY(csr_build_xw_plan(ctx, const_cast<padne_csr *>(k->L)));
        PADNE_TRY(products(k->c, k->w));                                                 // w = L c
    }
    if (uploader.joinable()) uploader.join();
    PADNE_TRY(up_rc);
    // 2. b = -P^T (r - L c) for every column, the extra right-hand sides, their norms
    const double *Lc = k->has_c ? k->w : nullptr;
    std::vector<double> norm2_buf((size_t)n_rhs + 8, 0.0);        // (one per right-hand side: any number of them)
    double *h_norm2 = norm2_buf.data();
    if (nf > 0) {
        hipLaunchKernelGGL(kkt_rhs, dim3(vgrid(nf)), dim3(256), 0, s, nf, N, n_cols, k->src_of, k->r, Lc, k->b);
        if (k->n_tied > 0)
            hipLaunchKernelGGL(kkt_rhs_tied, dim3(nblk(k->n_tied_groups), n_cols), dim3(256), 0, s, (int)k->n_tied_groups, nf, N,
                               n_cols, k->tied_gptr, k->tied_order, k->tied_member, k->tied_target, k->r, Lc, k->b);
        PADNE_HIP_CHECK(hipGetLastError());
        if (n_extra > 0) {
            long long *d_ptr = nullptr, *d_row = nullptr;
            double *d_val = nullptr;
            PADNE_TRY(sc.alloc(&d_ptr, (size_t)n_extra + 1));
            PADNE_TRY(sc.alloc(&d_row, (size_t)n_ex_entries));
            PADNE_TRY(sc.alloc(&d_val, (size_t)n_ex_entries));
            PADNE_HIP_CHECK(hipMemsetAsync(k->b + (long long)n_cols * nf, 0, sizeof(double) * (size_t)nf * (size_t)n_extra, s));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_ptr, extra_ptr, sizeof(long long) * (size_t)(n_extra + 1), hipMemcpyHostToDevice, s));
            if (n_ex_entries > 0) {
                PADNE_HIP_CHECK(hipMemcpyAsync(d_row, extra_row, sizeof(long long) * (size_t)n_ex_entries, hipMemcpyHostToDevice, s));
                PADNE_HIP_CHECK(hipMemcpyAsync(d_val, extra_val, sizeof(double) * (size_t)n_ex_entries, hipMemcpyHostToDevice, s));
            }
            hipLaunchKernelGGL(kkt_rhs_extra, dim3(1), dim3(1), 0, s, (int)n_extra, d_ptr, d_row, d_val, k->imap, nf,
                               k->b + (long long)n_cols * nf);
            PADNE_HIP_CHECK(hipGetLastError());
        }
        // norms of all right-hand sides (the tolerance rule below; zero right-hand sides are not solved for)
        const int g = vgrid(nf);
        for (int first = 0; first < n_rhs; first += 8) {
            const int cnt = std::min(8, n_rhs - first);
            hipLaunchKernelGGL(kkt_norm2, dim3(g, cnt), dim3(256), 0, s, nf, k->b + (long long)first * nf, ctx->partials);
            hipLaunchKernelGGL(kkt_fold, dim3(cnt), dim3(256), 0, s, ctx->partials, g, ctx->scalars + 32);
            PADNE_HIP_CHECK(hipGetLastError());
            if (cnt <= 7) {
                PADNE_TRY(read_back(ctx, ctx->scalars + 32, sizeof(double) * (size_t)cnt, h_norm2 + first));
            } else {
                PADNE_TRY(read_back2(ctx, ctx->scalars + 32, sizeof(double) * 4, h_norm2 + first, ctx->scalars + 36,
                                     sizeof(double) * 3, h_norm2 + first + 4));
                PADNE_TRY(read_back(ctx, ctx->scalars + 39, sizeof(double), h_norm2 + first + 7));
            }
        }
    }
    // 3. the reference judges a solve by the ABSOLUTE residual of the whole system (tests/test_solver.py:2083-2089): when
    //    rtol ||b|| is looser than the target the relative tolerance is tightened (never below what binary64 resolves); one
    //    tolerance for all columns, the tightest any of them needs
    double norm_max = 0.0;
    for (int j = 0; j < n_rhs; ++j) norm_max = std::max(norm_max, sqrt(h_norm2[j]));
    padne_solve_opts o = *opts;
    o.flags &= ~(1 | 4);                     // x0 = 0; the hierarchy was (re)built above
    if (abs_residual_target > 0.0 && norm_max > 0.0 && o.rtol * norm_max > abs_residual_target)
        o.rtol = std::max(abs_residual_target / norm_max, 2e-15);
    // right-hand sides that vanish are not solved for (y stays zero there)
    int rc_solve = PADNE_OK;
    auto solve_run = [&](const double *bb, double *yy, int cnt) -> int {
        padne_solve_info part;
        memset(&part, 0, sizeof(part));
        const int rc = padne_solve_spd_dev(ctx, k->A, bb, yy, cnt, &o, &part);
        if (rc != PADNE_OK && rc != PADNE_E_NOTCONVERGED) return rc;
        if (rc != PADNE_OK) rc_solve = rc;
        local.iterations += part.iterations;
        local.restarts += part.restarts;
        local.rel_residual = std::max(local.rel_residual, part.rel_residual);
        local.abs_residual = std::max(local.abs_residual, part.abs_residual);
        local.solve_seconds += part.solve_seconds;
        local.spmv_seconds = std::max(local.spmv_seconds, part.spmv_seconds);
        local.precond_fallbacks += part.precond_fallbacks;
        local.levels = part.levels;
        local.operator_complexity = part.operator_complexity;
        if (part.status != PADNE_OK) local.status = part.status;
        return PADNE_OK;
    };
    if (nf > 0) {
        PADNE_HIP_CHECK(hipMemsetAsync(k->y, 0, sizeof(double) * (size_t)nf * (size_t)n_rhs, s));
        std::vector<int> live;
        for (int j = 0; j < n_rhs; ++j)
            if (h_norm2[j] > 0.0) live.push_back(j);
        const bool gaps = !live.empty() && live.back() - live.front() + 1 != (int)live.size();
        if (n_cols > 1 && gaps) {
            // a block with zero columns among live ones: the live columns are packed, so that the lockstep grouping sees
            // all of them together, and their solutions are put back in place
            const int n_live = (int)live.size();
            double *bp = nullptr, *yp = nullptr;
            PADNE_TRY(sc.alloc(&bp, (size_t)n_live * (size_t)nf));
            PADNE_TRY(sc.alloc(&yp, (size_t)n_live * (size_t)nf));
            for (int q = 0; q < n_live; ++q)
                PADNE_HIP_CHECK(hipMemcpyAsync(bp + (long long)q * nf, k->b + (long long)live[q] * nf, sizeof(double) * (size_t)nf,
                                               hipMemcpyDeviceToDevice, s));
            PADNE_TRY(solve_run(bp, yp, n_live));
            for (int q = 0; q < n_live; ++q)
                PADNE_HIP_CHECK(hipMemcpyAsync(k->y + (long long)live[q] * nf, yp + (long long)q * nf, sizeof(double) * (size_t)nf,
                                               hipMemcpyDeviceToDevice, s));
        } else {
            // runs of live right-hand sides, one call each (they are one run unless a regulator's gain column projects to zero)
            int j = 0;
            while (j < n_rhs) {
                if (!(h_norm2[j] > 0.0)) {
                    ++j;
                    continue;
                }
                int j1 = j;
                while (j1 < n_rhs && h_norm2[j1] > 0.0) ++j1;
                PADNE_TRY(solve_run(k->b + (long long)j * nf, k->y + (long long)j * nf, j1 - j));
                j = j1;
            }
        }
    }
    local.precond_setup_seconds = setup_s;
    // 4. v = c + P y (multipliers still zero), Z_k = P z_k (once per block), and the KCL residual rows the host peels the
    //    multipliers from
    const double *c = k->has_c ? k->c : nullptr;
    if (last_w > last) PADNE_HIP_CHECK(hipMemsetAsync(k->v + last_off, 0, sizeof(double) * (size_t)N * (size_t)last_w, s));
    hipLaunchKernelGGL(kkt_expand, dim3(vgrid(N)), dim3(256), 0, s, N, n_cols, k->imap, k->y, nf, c, k->v);
    for (int j = 0; j < n_extra; ++j)
        hipLaunchKernelGGL(kkt_expand, dim3(vgrid(N)), dim3(256), 0, s, N, 1, k->imap, k->y + (long long)(n_cols + j) * nf, nf,
                           (const double *)nullptr, k->Z + (long long)j * N);
    PADNE_HIP_CHECK(hipGetLastError());
    if (n_probe > 0) {
        long long *d_idx = nullptr;
        double *d_out = nullptr;
        PADNE_TRY(sc.alloc(&d_idx, (size_t)n_probe));
        PADNE_TRY(sc.alloc(&d_out, (size_t)n_probe * (size_t)n_rhs));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_idx, probe_idx, sizeof(long long) * (size_t)n_probe, hipMemcpyHostToDevice, s));
        PADNE_TRY(csr_build_xw_plan(ctx, const_cast<padne_csr *>(k->L)));
        PADNE_TRY(products(k->v, k->w));                                                               // L v
        hipLaunchKernelGGL(kkt_rho_probe, dim3(nblk(n_probe), n_cols), dim3(256), 0, s, (int)n_probe, N, n_cols, d_idx, k->r, k->w,
                           d_out);                                                                     // rho = r - L v
        for (int j = 0; j < n_extra; ++j) {
            PADNE_TRY(launch_spmv(ctx, k->L, k->Z + (long long)j * N, k->w, nullptr, nullptr, nullptr));  // L Z_k
            hipLaunchKernelGGL(kkt_gather_f64, dim3(nblk(n_probe)), dim3(256), 0, s, (int)n_probe, d_idx, k->w,
                               d_out + (size_t)(n_cols + j) * (size_t)n_probe);
        }
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_HIP_CHECK(hipMemcpyAsync(probe_out, d_out, sizeof(double) * (size_t)n_probe * (size_t)n_rhs, hipMemcpyDeviceToHost, s));
    }
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    k->solved = true;
    if (info) *info = local;
    return rc_solve;
}

// Stage 2 for the block of the last stage 1
static int kkt_finish_block(padne_ctx *ctx, padne_kkt *k, const int n_cols, int32_t n_extra, const double *extra_coeff,
                            int64_t n_mult, const int64_t *mult_idx, const double *mult_val, double *v_host,
                            double *residual_norms_out) {
    PADNE_REQUIRE(ctx && k && v_host && residual_norms_out, "null argument");
    PADNE_REQUIRE(k->ctx == ctx && k->solved, "padne_kkt_finish follows padne_kkt_solve on the same plan");
    PADNE_REQUIRE(n_cols == k->n_cols, "as many columns as the solve had");
    PADNE_REQUIRE(n_extra == k->n_extra && (n_extra == 0 || extra_coeff), "one coefficient per extra right-hand side");
    PADNE_REQUIRE(n_mult >= 0 && (n_mult == 0 || (mult_idx && mult_val)), "multipliers");
    const long long N = k->N;
    for (int64_t j = 0; j < n_mult; ++j) PADNE_REQUIRE(mult_idx[j] >= 0 && mult_idx[j] < N, "multiplier index out of range");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    // the result travels home in the caller's layout: when the products' layout differs it is written to c (free now) as well
    const bool same_layout = kkt_block_width(n_cols) == n_cols && n_cols <= 8;
    double *v_out = same_layout ? k->v : k->c;
    double *v_caller = same_layout ? nullptr : k->c;
    if (n_extra > 0 || !same_layout) {
        double *d_coeff = nullptr;
        if (n_extra > 0) {
            PADNE_TRY(sc.alloc(&d_coeff, (size_t)n_extra * (size_t)n_cols));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_coeff, extra_coeff, sizeof(double) * (size_t)n_extra * (size_t)n_cols,
                                           hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(kkt_add_extras, dim3(vgrid(N)), dim3(256), 0, s, N, n_cols, (int)n_extra, (const double *)d_coeff, k->Z,
                           k->v, v_caller);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    if (n_mult > 0) {
        long long *d_idx = nullptr;
        double *d_val = nullptr;
        PADNE_TRY(sc.alloc(&d_idx, (size_t)n_mult));
        PADNE_TRY(sc.alloc(&d_val, (size_t)n_mult * (size_t)n_cols));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_idx, mult_idx, sizeof(long long) * (size_t)n_mult, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_val, mult_val, sizeof(double) * (size_t)n_mult * (size_t)n_cols, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(kkt_scatter_block, dim3(nblk(n_mult), n_cols), dim3(256), 0, s, (int)n_mult, N, n_cols, d_idx, d_val, k->v,
                           v_caller);
        PADNE_HIP_CHECK(hipGetLastError());
    }
    // V is final: it travels home on the copy streams while the main stream evaluates ||L v_j - r_j|| (solver.py:775)
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    int down_rc = PADNE_OK;
    std::thread downloader([&]() {
        (void)hipSetDevice(ctx->device);
        down_rc = parallel_copy(k, v_host, v_out, sizeof(double) * (size_t)N * (size_t)n_cols, hipMemcpyDeviceToHost);
    });
    struct Join {
        std::thread &t;
        ~Join() { if (t.joinable()) t.join(); }
    } join_guard{downloader};
    std::vector<double> norm2((size_t)n_cols, 0.0);
    if (N > 0) {
        double *d_part = nullptr, *d_norm2 = nullptr;
        PADNE_TRY(sc.alloc(&d_part, (size_t)n_cols * kMaxPartials));
        PADNE_TRY(sc.alloc(&d_norm2, (size_t)n_cols));
        PADNE_TRY(csr_build_xw_plan(ctx, const_cast<padne_csr *>(k->L)));
        PADNE_TRY(kkt_products(ctx, k, n_cols, k->v, k->w));      // L v
        const int g = vgrid(N);
        hipLaunchKernelGGL(kkt_diff2, dim3(g, n_cols), dim3(256), 0, s, N, n_cols, k->w, k->r, d_part);
        hipLaunchKernelGGL(kkt_fold, dim3(n_cols), dim3(256), 0, s, d_part, g, d_norm2);
        PADNE_HIP_CHECK(hipGetLastError());
        PADNE_TRY(read_back(ctx, d_norm2, sizeof(double) * (size_t)n_cols, norm2.data()));
    }
    downloader.join();
    PADNE_TRY(down_rc);
    for (int j = 0; j < n_cols; ++j) residual_norms_out[j] = sqrt(norm2[(size_t)j]);
    k->solved = false;
    k->finished = true;
    k->v_final = v_out;
    k->finished_cols = n_cols;
    return PADNE_OK;
}

extern "C" int padne_kkt_solve(padne_ctx *ctx, padne_kkt *k, const double *r_host, int64_t n_known, const int64_t *known_idx,
                               const double *known_val, int32_t n_extra, const int64_t *extra_ptr, const int64_t *extra_row,
                               const double *extra_val, int64_t n_probe, const int64_t *probe_idx, double *probe_out,
                               const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info) {
    KktRhs rhs;
    rhs.dense = r_host;
    PADNE_REQUIRE(r_host, "null argument");
    return kkt_solve_block(ctx, k, 1, rhs, n_known, known_idx, known_val, n_extra, extra_ptr, extra_row, extra_val, n_probe,
                           probe_idx, probe_out, opts, abs_residual_target, info);
}

extern "C" int padne_kkt_solve_block(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, const double *r_host, int64_t n_known,
                                     const int64_t *known_idx, const double *known_val, int32_t n_extra, const int64_t *extra_ptr,
                                     const int64_t *extra_row, const double *extra_val, int64_t n_probe, const int64_t *probe_idx,
                                     double *probe_out, const padne_solve_opts *opts, double abs_residual_target,
                                     padne_solve_info *info) {
    KktRhs rhs;
    rhs.dense = r_host;
    PADNE_REQUIRE(r_host, "null argument");
    return kkt_solve_block(ctx, k, n_cols, rhs, n_known, known_idx, known_val, n_extra, extra_ptr, extra_row, extra_val, n_probe,
                           probe_idx, probe_out, opts, abs_residual_target, info);
}

extern "C" int padne_kkt_solve_block_dev(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, const void *r_dev, int64_t n_known,
                                         const int64_t *known_idx, const double *known_val, int32_t n_extra, const int64_t *extra_ptr,
                                         const int64_t *extra_row, const double *extra_val, int64_t n_probe, const int64_t *probe_idx,
                                         double *probe_out, const padne_solve_opts *opts, double abs_residual_target,
                                         padne_solve_info *info) {
    KktRhs rhs;
    rhs.dense_dev = (const double *)r_dev;
    PADNE_REQUIRE(r_dev, "null argument");
    return kkt_solve_block(ctx, k, n_cols, rhs, n_known, known_idx, known_val, n_extra, extra_ptr, extra_row, extra_val, n_probe,
                           probe_idx, probe_out, opts, abs_residual_target, info);
}

extern "C" int padne_kkt_finish(padne_ctx *ctx, padne_kkt *k, int32_t n_extra, const double *extra_coeff, int64_t n_mult,
                                const int64_t *mult_idx, const double *mult_val, double *v_host, double *residual_norm_out) {
    return kkt_finish_block(ctx, k, 1, n_extra, extra_coeff, n_mult, mult_idx, mult_val, v_host, residual_norm_out);
}

extern "C" int padne_kkt_finish_block(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int32_t n_extra, const double *extra_coeff,
                                      int64_t n_mult, const int64_t *mult_idx, const double *mult_val, double *v_host,
                                      double *residual_norms_out) {
    return kkt_finish_block(ctx, k, n_cols, n_extra, extra_coeff, n_mult, mult_idx, mult_val, v_host, residual_norms_out);
}

extern "C" int padne_kkt_solve_block_coo(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int64_t n_entries, const int64_t *r_row,
                                         const int32_t *r_col, const double *r_val, int64_t n_known, const int64_t *known_idx,
                                         const double *known_val, int32_t n_extra, const int64_t *extra_ptr, const int64_t *extra_row,
                                         const double *extra_val, int64_t n_probe, const int64_t *probe_idx, double *probe_out,
                                         const padne_solve_opts *opts, double abs_residual_target, padne_solve_info *info) {
    KktRhs rhs;
    rhs.n_entries = n_entries;
    rhs.row = r_row;
    rhs.col = r_col;
    rhs.val = r_val;
    return kkt_solve_block(ctx, k, n_cols, rhs, n_known, known_idx, known_val, n_extra, extra_ptr, extra_row, extra_val, n_probe,
                           probe_idx, probe_out, opts, abs_residual_target, info);
}

// What every post-processing entry asks before it reads the V that stage 2 left on the device: the plan is the context's, a
// block is finished (`entry` names the caller in the message) and has n_cols columns, and the system matrix carries a mesh
// of no more vertices than the system has unknowns.
static int require_finished_block(const char *entry, padne_ctx *ctx, const padne_kkt *k, int32_t n_cols) {
    PADNE_REQUIRE(ctx && k, "null argument");
    PADNE_REQUIRE(k->ctx == ctx, "the plan belongs to another context");
    PADNE_REQUIRE(k->finished && k->v_final != nullptr,
                  (std::string(entry) + " follows padne_kkt_finish_block, with no solve on the plan in between").c_str());
    PADNE_REQUIRE(n_cols == k->finished_cols, "as many columns as the finished block has");
    const padne_csr *L = k->L;
    PADNE_REQUIRE(L->mesh_n_mesh > 0 && L->mesh_xy != nullptr,
                  "the system matrix does not carry a mesh (only padne_assemble_system keeps it)");
    PADNE_REQUIRE(L->mesh_n_vert <= k->N, "the mesh has more vertices than the system has unknowns");
    return PADNE_OK;
}

// The finished block of a plan for a consumer in another translation unit (thermal.hip): after the same checks, the V that
// stage 2 left on the device ([N][n_cols] row-major), N and the system the plan was made for.
namespace padne {
int kkt_finished_block(const char *entry, padne_ctx *ctx, const padne_kkt *k, int32_t n_cols, const double **V_out, long long *N_out,
                       const padne_csr **L_out) {
    PADNE_TRY(require_finished_block(entry, ctx, k, n_cols));
    *V_out = k->v_final;
    *N_out = k->N;
    *L_out = k->L;
    return PADNE_OK;
}
}  // namespace padne

// The flag a face kernel sets when a triangle names a vertex outside its mesh: a zeroed device int from `sc` ...
static int bad_flag_alloc(Scratch &sc, hipStream_t s, int **d_bad) {
    PADNE_TRY(sc.alloc(d_bad, 1));
    PADNE_HIP_CHECK(hipMemsetAsync(*d_bad, 0, sizeof(int), s));
    return PADNE_OK;
}

// ... and its read-back: waits for everything queued on `s` (the caller's own small copies home included)
static int bad_flag_check(hipStream_t s, const int *d_bad) {
    int h_bad = 0;
    PADNE_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("invalid argument: triangle index out of range");
        return PADNE_E_INVALID;
    }
    return PADNE_OK;
}

// sigma |grad V|^2 of every column of the finished block, from the V that stage 2 left on the device: one launch over the
// triangles (power_density_block_kernel), then [n_cols][n_tri] home on the copy streams
extern "C" int padne_kkt_power_density_block(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, double *out_host) {
    PADNE_TRY(require_finished_block("padne_kkt_power_density_block", ctx, k, n_cols));
    const padne_csr *L = k->L;
    const long long n_tri = L->mesh_n_tri;
    if (n_tri == 0) return PADNE_OK;
    PADNE_REQUIRE(out_host != nullptr, "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    double *d_out = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_out, (size_t)n_tri * (size_t)n_cols));
    PADNE_TRY(bad_flag_alloc(sc, s, &d_bad));
    PADNE_TRY(launch_power_density_block(ctx, L, n_cols, k->v_final, d_out, d_bad));
    PADNE_TRY(bad_flag_check(s, d_bad));
    return parallel_copy(k, out_host, d_out, sizeof(double) * (size_t)n_tri * (size_t)n_cols, hipMemcpyDeviceToHost);
}

// Element cases (cases.hip; DESIGN.md, "Element cases"): V' = V W^T for the CSR weights W [n_out][n_cols], out of place into
// a block of its own that takes the finished block's place.  The weights are checked here, before the device is touched.
extern "C" int padne_kkt_combine_block(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int32_t n_out, const int64_t *w_ptr,
                                       const int32_t *w_col, const double *w_val, double *v_host) {
    PADNE_TRY(require_finished_block("padne_kkt_combine_block", ctx, k, n_cols));
    PADNE_REQUIRE(n_out >= 1 && n_out <= 4096, "between 1 and 4096 combined columns");
    PADNE_REQUIRE(w_ptr != nullptr, "null argument");
    PADNE_REQUIRE(w_ptr[0] == 0, "the weights' row pointer starts at 0");
    for (int c = 0; c < n_out; ++c)
        PADNE_REQUIRE(w_ptr[c + 1] >= w_ptr[c] && w_ptr[c + 1] - w_ptr[c] <= n_cols, "the weights' row pointer must be monotone");
    const long long nnz = w_ptr[n_out];
    PADNE_REQUIRE(nnz == 0 || (w_col && w_val), "null argument");
    std::vector<int> h_ptr((size_t)n_out + 1);
    for (int c = 0; c <= n_out; ++c) h_ptr[(size_t)c] = (int)w_ptr[c];
    for (int c = 0; c < n_out; ++c)
        for (long long e = w_ptr[c]; e < w_ptr[c + 1]; ++e) {
            PADNE_REQUIRE(w_col[e] >= 0 && w_col[e] < n_cols, "weight column out of range");
            PADNE_REQUIRE(e == w_ptr[c] || w_col[e] > w_col[e - 1], "the columns of a row of weights must be strictly ascending");
            PADNE_REQUIRE(std::isfinite(w_val[e]), "weights must be finite");
        }
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const long long N = k->N;
    Scratch sc(ctx);
    int *d_ptr = nullptr, *d_col = nullptr;
    double *d_val = nullptr, *d_new = nullptr;
    PADNE_TRY(sc.alloc(&d_ptr, (size_t)n_out + 1));
    PADNE_TRY(sc.alloc(&d_col, (size_t)nnz));
    PADNE_TRY(sc.alloc(&d_val, (size_t)nnz));
    PADNE_TRY(sc.alloc(&d_new, (size_t)(N > 0 ? N : 1) * (size_t)n_out));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_ptr, h_ptr.data(), sizeof(int) * ((size_t)n_out + 1), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        PADNE_HIP_CHECK(hipMemcpyAsync(d_col, w_col, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_val, w_val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, s));
    }
    PADNE_TRY(launch_combine_block(ctx, N, n_cols, n_out, nnz, d_ptr, d_col, d_val, k->v_final, d_new));
    PADNE_HIP_CHECK(hipStreamSynchronize(s));           // the host arrays above are the caller's and h_ptr is this frame's
    sc.disown(d_new);
    if (k->combined != nullptr) pool_free(ctx, k->combined);       // a block combined before: it was this call's input
    k->combined = d_new;
    k->v_final = d_new;
    k->finished_cols = n_out;
    if (v_host != nullptr && N > 0)
        PADNE_TRY(parallel_copy(k, v_host, d_new, sizeof(double) * (size_t)N * (size_t)n_out, hipMemcpyDeviceToHost));
    return PADNE_OK;
}

// the first 256-triangle tile of every mesh of `L`, from its triangle offsets: tile[m] .. tile[m + 1] are mesh m's tiles, the
// layout of sensitivity_block_kernel and the current kernels
static int mesh_tiles(padne_ctx *ctx, const padne_csr *L, std::vector<long long> &tile) {
    const int n_mesh = (int)L->mesh_n_mesh;
    std::vector<long long> toff((size_t)n_mesh + 1);
    tile.assign((size_t)n_mesh + 1, 0);
    PADNE_HIP_CHECK(hipMemcpyAsync(toff.data(), L->mesh_toff, sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyDeviceToHost,
                                   ctx->stream));
    PADNE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < n_mesh; ++m) {
        PADNE_REQUIRE(toff[(size_t)m + 1] >= toff[(size_t)m], "mesh triangle offsets");
        tile[(size_t)m + 1] = tile[(size_t)m] + (toff[(size_t)m + 1] - toff[(size_t)m] + 255) / 256;
    }
    PADNE_REQUIRE(tile[(size_t)n_mesh] <= 0x7fffffffLL, "too many triangles for one launch");
    return PADNE_OK;
}

// dJ_j / dsigma of every face for the adjoints lambda_j = sum_m weights[j][m] V[:, m] of the finished block, and the power
// density of its column 0: the tiles of each mesh are laid out here from the mesh's triangle offsets, then one launch over
// them (sensitivity_block_kernel) and one fold of the per-tile partials per (mesh, objective); the three results go home
extern "C" int padne_kkt_sensitivity_block(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int32_t n_obj, const double *weights,
                                           double *power_out, double *density_out, double *mesh_total_out) {
    PADNE_TRY(require_finished_block("padne_kkt_sensitivity_block", ctx, k, n_cols));
    PADNE_REQUIRE(n_obj >= 1 && n_obj <= 4096, "between 1 and 4096 objectives");
    PADNE_REQUIRE(weights && mesh_total_out, "null argument");
    for (long long e = 0; e < (long long)n_obj * n_cols; ++e) PADNE_REQUIRE(std::isfinite(weights[e]), "weights must be finite");
    const padne_csr *L = k->L;
    const long long n_tri = L->mesh_n_tri;
    const int n_mesh = (int)L->mesh_n_mesh;
    PADNE_REQUIRE(n_tri == 0 || (power_out && density_out), "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<long long> tile;
    PADNE_TRY(mesh_tiles(ctx, L, tile));
    Scratch sc(ctx);
    double *d_w = nullptr, *d_power = nullptr, *d_density = nullptr, *d_total = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_w, (size_t)n_obj * (size_t)n_cols));
    PADNE_TRY(sc.alloc(&d_power, (size_t)n_tri));
    PADNE_TRY(sc.alloc(&d_density, (size_t)n_tri * (size_t)n_obj));
    PADNE_TRY(sc.alloc(&d_total, (size_t)n_mesh * (size_t)n_obj));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_w, weights, sizeof(double) * (size_t)n_obj * (size_t)n_cols, hipMemcpyHostToDevice, s));
    PADNE_TRY(bad_flag_alloc(sc, s, &d_bad));
    PADNE_TRY(launch_sensitivity_block(ctx, L, tile.data(), n_cols, n_obj, d_w, k->v_final, d_power, d_density, d_total, d_bad));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_total_out, d_total, sizeof(double) * (size_t)n_mesh * (size_t)n_obj, hipMemcpyDeviceToHost, s));
    if (n_tri > 0) PADNE_HIP_CHECK(hipMemcpyAsync(power_out, d_power, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost, s));
    PADNE_TRY(bad_flag_check(s, d_bad));
    if (n_tri == 0) return PADNE_OK;
    return parallel_copy(k, density_out, d_density, sizeof(double) * (size_t)n_tri * (size_t)n_obj, hipMemcpyDeviceToHost);
}

// Does the segment c = (start x, y, end x, y) meet the box (x_min, y_min, x_max, y_max)?  Separating axes: x, y and the
// segment's normal.  The box is padded by far more than the rounding of orient(), so that no tile holding an edge the cut
// kernel counts as crossing is left out; a tile the segment only grazes adds work, not current.
static bool segment_meets_box(const double *c, const double *box) {
    double scale = 1.0;
    for (int q = 0; q < 4; ++q) scale = std::max(scale, std::max(std::fabs(c[q]), std::fabs(box[q])));
    const double pad = 1e-9 * scale;
    const double x0 = box[0] - pad, y0 = box[1] - pad, x1 = box[2] + pad, y1 = box[3] + pad;
    if (std::max(c[0], c[2]) < x0 || std::min(c[0], c[2]) > x1 || std::max(c[1], c[3]) < y0 || std::min(c[1], c[3]) > y1)
        return false;
    const double dx = c[2] - c[0], dy = c[3] - c[1];
    const double cx[4] = {x0, x1, x1, x0}, cy[4] = {y0, y0, y1, y1};
    int pos = 0, neg = 0;
    for (int q = 0; q < 4; ++q) {
        const double o = dx * (cy[q] - c[1]) - dy * (cx[q] - c[0]);
        pos += o > 0;
        neg += o < 0;
    }
    return pos < 4 && neg < 4;
}

// the end points of n_cut cuts, cut_xy[c] = (start x, y, end x, y): finite, and start != end
static int check_cut_segments(int n_cut, const double *cut_xy) {
    for (int c = 0; c < n_cut; ++c) {
        const double *p = cut_xy + 4 * (size_t)c;
        for (int q = 0; q < 4; ++q) PADNE_REQUIRE(std::isfinite(p[q]), "cut end points must be finite");
        PADNE_REQUIRE(p[0] != p[2] || p[1] != p[3], "a cut's start and end must differ");
    }
    return PADNE_OK;
}

// the (cut, tile) pairs, by cut and then by tile: the tiles of the meshes on the cut's layer whose box the segment meets;
// pair_off[c] .. pair_off[c + 1] are cut c's pairs
static void list_cut_pairs(int n_cut, int n_mesh, const int32_t *mesh_layer, const int32_t *cut_layer, const double *cut_xy,
                           const std::vector<long long> &tile, const std::vector<double> &box, std::vector<int> &pair_cut,
                           std::vector<long long> &pair_tile, std::vector<long long> &pair_off) {
    pair_cut.clear();
    pair_tile.clear();
    pair_off.assign((size_t)n_cut + 1, 0);
    for (int c = 0; c < n_cut; ++c) {
        for (int m = 0; m < n_mesh; ++m) {
            if (mesh_layer[m] != cut_layer[c]) continue;
            for (long long b = tile[(size_t)m]; b < tile[(size_t)m + 1]; ++b)
                if (segment_meets_box(cut_xy + 4 * (size_t)c, box.data() + 4 * (size_t)b)) {
                    pair_cut.push_back(c);
                    pair_tile.push_back(b);
                }
        }
        pair_off[(size_t)c + 1] = (long long)pair_tile.size();
    }
}

// The currents of the n_report leading columns of the finished block and their envelope ("Currents"): J = -sigma
// grad V and |J| of every face, the largest |J| and the power of every mesh, and the current through each cut.  One launch
// over the tiles of sensitivity_block_kernel's layout writes J, |J|, the envelope, per-tile maxima and powers and per-tile
// bounding boxes, and one fold per (mesh, column) reduces the tiles.  The boxes come home; the (cut, tile) pairs whose box
// the cut's segment meets are listed here, on the host; one workgroup per pair and one fold per (cut, column) give the cut
// currents.  J_out and mag_out, env_out and env_case_out, mesh_power_out: null for an output that is not wanted, which is
// then neither written on the device nor copied home.  No floating-point atomics: two calls give the same bits.
static int kkt_currents(const char *entry, padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int32_t n_report, int64_t n_tri,
                        int32_t n_mesh, const int32_t *mesh_layer, int32_t n_cut, const int32_t *cut_layer, const double *cut_xy,
                        double *J_out, double *mag_out, double *env_out, int32_t *env_case_out, double *mesh_max_out,
                        int64_t *mesh_face_out, double *mesh_power_out, double *cut_out) {
    PADNE_TRY(require_finished_block(entry, ctx, k, n_cols));
    PADNE_REQUIRE(n_cut >= 0 && n_cut <= 4096, "between 0 and 4096 cuts");
    PADNE_REQUIRE(mesh_max_out && mesh_face_out, "null argument");
    PADNE_REQUIRE(n_cut == 0 || (mesh_layer && cut_layer && cut_xy && cut_out), "null argument");
    PADNE_REQUIRE((J_out == nullptr) == (mag_out == nullptr), "J_out and mag_out are given or left out together");
    PADNE_REQUIRE((env_out == nullptr) == (env_case_out == nullptr), "env_out and env_case_out are given or left out together");
    PADNE_TRY(check_cut_segments(n_cut, cut_xy));
    const padne_csr *L = k->L;
    PADNE_REQUIRE(n_tri == L->mesh_n_tri && n_mesh == L->mesh_n_mesh, "n_tri and n_mesh must be those of the system's mesh");
    const bool fields = J_out != nullptr, envelope = env_out != nullptr, power = mesh_power_out != nullptr;
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<long long> tile;
    PADNE_TRY(mesh_tiles(ctx, L, tile));
    const long long n_blocks = tile[(size_t)n_mesh];
    const size_t nb = (size_t)(n_blocks > 0 ? n_blocks : 1), nt = (size_t)(n_tri > 0 ? n_tri : 1), nc = (size_t)n_report;
    Scratch sc(ctx);
    long long *d_tile = nullptr, *d_mface = nullptr;
    double *d_J = nullptr, *d_mag = nullptr, *d_env = nullptr, *d_box = nullptr, *d_mmax = nullptr, *d_mpow = nullptr;
    int *d_case = nullptr, *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_tile, (size_t)n_mesh + 1));
    if (fields) {
        PADNE_TRY(sc.alloc(&d_J, 2 * nt * nc));
        PADNE_TRY(sc.alloc(&d_mag, nt * nc));
    }
    if (envelope) {
        PADNE_TRY(sc.alloc(&d_env, nt));
        PADNE_TRY(sc.alloc(&d_case, nt));
    }
    PADNE_TRY(sc.alloc(&d_box, 4 * nb));
    PADNE_TRY(sc.alloc(&d_mmax, (size_t)n_mesh * nc));
    PADNE_TRY(sc.alloc(&d_mface, (size_t)n_mesh * nc));
    if (power) PADNE_TRY(sc.alloc(&d_mpow, (size_t)n_mesh * nc));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_tile, tile.data(), sizeof(long long) * ((size_t)n_mesh + 1), hipMemcpyHostToDevice, s));
    PADNE_TRY(bad_flag_alloc(sc, s, &d_bad));
    PADNE_TRY(launch_current_faces(ctx, L, d_tile, n_blocks, n_cols, n_report, k->v_final, d_J, d_mag, d_env, d_case, d_box, d_mmax,
                                   d_mface, d_mpow, d_bad));
    if (n_cut > 0) {
        std::vector<double> box(4 * nb);
        if (n_blocks > 0)
            PADNE_HIP_CHECK(hipMemcpyAsync(box.data(), d_box, sizeof(double) * 4 * (size_t)n_blocks, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));
        std::vector<int> pair_cut;
        std::vector<long long> pair_tile, pair_off;
        list_cut_pairs(n_cut, n_mesh, mesh_layer, cut_layer, cut_xy, tile, box, pair_cut, pair_tile, pair_off);
        const long long n_pairs = (long long)pair_tile.size();
        PADNE_REQUIRE(n_pairs <= 0x7fffffffLL, "too many (cut, tile) pairs for one launch");
        const size_t np = (size_t)(n_pairs > 0 ? n_pairs : 1);
        double *d_cut_xy = nullptr, *d_cut = nullptr;
        int *d_pair_cut = nullptr;
        long long *d_pair_tile = nullptr;
        PADNE_TRY(sc.alloc(&d_cut_xy, 4 * (size_t)n_cut));
        PADNE_TRY(sc.alloc(&d_cut, (size_t)n_cut * nc));
        PADNE_TRY(sc.alloc(&d_pair_cut, np));
        PADNE_TRY(sc.alloc(&d_pair_tile, np));
        PADNE_HIP_CHECK(hipMemcpyAsync(d_cut_xy, cut_xy, sizeof(double) * 4 * (size_t)n_cut, hipMemcpyHostToDevice, s));
        if (n_pairs > 0) {
            PADNE_HIP_CHECK(hipMemcpyAsync(d_pair_cut, pair_cut.data(), sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
            PADNE_HIP_CHECK(hipMemcpyAsync(d_pair_tile, pair_tile.data(), sizeof(long long) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
        }
        PADNE_TRY(launch_current_cuts(ctx, L, d_tile, n_cols, n_report, k->v_final, n_cut, d_cut_xy, n_pairs, d_pair_cut, d_pair_tile,
                                      pair_off.data(), d_cut, d_bad));
        PADNE_HIP_CHECK(hipMemcpyAsync(cut_out, d_cut, sizeof(double) * (size_t)n_cut * nc, hipMemcpyDeviceToHost, s));
        PADNE_HIP_CHECK(hipStreamSynchronize(s));       // (the copies read the host vectors above before they go)
    }
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_mmax, sizeof(double) * (size_t)n_mesh * nc, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_face_out, d_mface, sizeof(long long) * (size_t)n_mesh * nc, hipMemcpyDeviceToHost, s));
    if (power)
        PADNE_HIP_CHECK(hipMemcpyAsync(mesh_power_out, d_mpow, sizeof(double) * (size_t)n_mesh * nc, hipMemcpyDeviceToHost, s));
    PADNE_TRY(bad_flag_check(s, d_bad));
    if (n_tri == 0) return PADNE_OK;
    if (fields) {
        PADNE_TRY(parallel_copy(k, J_out, d_J, sizeof(double) * 2 * (size_t)n_tri * nc, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, mag_out, d_mag, sizeof(double) * (size_t)n_tri * nc, hipMemcpyDeviceToHost));
    }
    if (envelope) {
        PADNE_TRY(parallel_copy(k, env_out, d_env, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, env_case_out, d_case, sizeof(int32_t) * (size_t)n_tri, hipMemcpyDeviceToHost));
    }
    return PADNE_OK;
}

// the currents of column 0 of the finished block: kkt_currents with one reported column, no envelope and no power
extern "C" int padne_kkt_current_report(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int64_t n_tri, int32_t n_mesh,
                                        const int32_t *mesh_layer, int32_t n_cut, const int32_t *cut_layer, const double *cut_xy,
                                        double *J_out, double *mag_out, double *mesh_max_out, int64_t *mesh_face_out,
                                        double *cut_out) {
    PADNE_REQUIRE(n_tri == 0 || (J_out && mag_out), "null argument");
    return kkt_currents("padne_kkt_current_report", ctx, k, n_cols, 1, n_tri, n_mesh, mesh_layer, n_cut, cut_layer, cut_xy, J_out,
                        mag_out, nullptr, nullptr, mesh_max_out, mesh_face_out, nullptr, cut_out);
}

// the currents of every column of the finished block and their envelope ("Load-case currents"); with J_out and
// mag_out null no per-column field is written on the device or copied home, with env_out and env_case_out null no envelope
extern "C" int padne_kkt_current_cases(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int64_t n_tri, int32_t n_mesh,
                                       const int32_t *mesh_layer, int32_t n_cut, const int32_t *cut_layer, const double *cut_xy,
                                       double *J_out, double *mag_out, double *env_out, int32_t *env_case_out,
                                       double *mesh_max_out, int64_t *mesh_face_out, double *mesh_power_out, double *cut_out) {
    PADNE_REQUIRE(mesh_power_out != nullptr, "null argument");
    return kkt_currents("padne_kkt_current_cases", ctx, k, n_cols, n_cols, n_tri, n_mesh, mesh_layer, n_cut, cut_layer, cut_xy, J_out,
                        mag_out, env_out, env_case_out, mesh_max_out, mesh_face_out, mesh_power_out, cut_out);
}

// The gradient-recovery error estimate of column 0 of the finished block (error.hip; DESIGN.md, "Error estimate"): the
// vertex -> faces lists of L's mesh are built on the first call and stay with the plan, then three passes over the mesh and
// one fold per mesh.  No floating-point atomics: two calls give the same bits.  Only the results cross PCIe.
extern "C" int padne_kkt_error_estimate(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int64_t n_tri, int64_t n_vert, int32_t n_mesh,
                                        double *G_out, double *eta_out, double *mesh_error_out, double *mesh_power_out,
                                        double *mesh_max_out, int64_t *mesh_face_out) {
    PADNE_TRY(require_finished_block("padne_kkt_error_estimate", ctx, k, n_cols));
    PADNE_REQUIRE(mesh_error_out && mesh_power_out && mesh_max_out && mesh_face_out, "null argument");
    const padne_csr *L = k->L;
    PADNE_REQUIRE(n_tri == L->mesh_n_tri && n_vert == L->mesh_n_vert && n_mesh == L->mesh_n_mesh,
                  "n_tri, n_vert and n_mesh must be those of the system's mesh");
    PADNE_REQUIRE((n_tri == 0 || eta_out) && (n_vert == 0 || G_out), "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nt = (size_t)(n_tri > 0 ? n_tri : 1), nv = (size_t)(n_vert > 0 ? n_vert : 1);
    Scratch sc(ctx);
    double *d_G = nullptr, *d_eta = nullptr, *d_E = nullptr, *d_P = nullptr, *d_max = nullptr;
    long long *d_face = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_G, 2 * nv));
    PADNE_TRY(sc.alloc(&d_eta, nt));
    PADNE_TRY(sc.alloc(&d_E, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_P, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_max, (size_t)n_mesh));
    PADNE_TRY(sc.alloc(&d_face, (size_t)n_mesh));
    PADNE_TRY(bad_flag_alloc(sc, s, &d_bad));
    PADNE_TRY(csr_error_estimate(ctx, L, &k->err_vptr, &k->err_vface, n_cols, k->v_final, d_G, d_eta, d_E, d_P, d_max, d_face, d_bad));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_error_out, d_E, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_power_out, d_P, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, d_max, sizeof(double) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_face_out, d_face, sizeof(long long) * (size_t)n_mesh, hipMemcpyDeviceToHost, s));
    PADNE_TRY(bad_flag_check(s, d_bad));
    if (n_vert > 0) PADNE_TRY(parallel_copy(k, G_out, d_G, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyDeviceToHost));
    if (n_tri > 0) PADNE_TRY(parallel_copy(k, eta_out, d_eta, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost));
    return PADNE_OK;
}

// The goal-oriented (dual-weighted) error estimate of the finished block (goal.hip; DESIGN.md, "Goal-oriented error"): field 0
// is column 0, field 1 + j the adjoint sum_m weights[j][m] V[:, m], as padne_kkt_sensitivity_block takes the weights.  The
// vertex -> faces lists are those of padne_kkt_error_estimate, built by whichever of the two is called first and kept with
// the plan; the field-0 results are that entry's bits.  Only the results cross PCIe.
extern "C" int padne_kkt_goal_error(padne_ctx *ctx, padne_kkt *k, int32_t n_cols, int32_t n_obj, const double *weights, int64_t n_tri,
                                    int64_t n_vert, int32_t n_mesh, double *power_out, double *G_out, double *eta_out,
                                    double *mesh_error_out, double *mesh_power_out, double *mesh_max_out, int64_t *mesh_face_out, double *dual_eta_out,
                                    double *delta_out, double *omega_out, double *mesh_omega_out, double *mesh_delta_out,
                                    double *mesh_top_out, int64_t *mesh_top_face_out) {
    PADNE_TRY(require_finished_block("padne_kkt_goal_error", ctx, k, n_cols));
    PADNE_REQUIRE(n_obj >= 1 && n_obj <= 4096, "between 1 and 4096 objectives");
    PADNE_REQUIRE(weights, "null argument");
    for (long long e = 0; e < (long long)n_obj * n_cols; ++e) PADNE_REQUIRE(std::isfinite(weights[e]), "weights must be finite");
    PADNE_REQUIRE(mesh_error_out && mesh_power_out && mesh_max_out && mesh_face_out, "null argument");
    PADNE_REQUIRE(mesh_omega_out && mesh_delta_out && mesh_top_out && mesh_top_face_out, "null argument");
    const padne_csr *L = k->L;
    PADNE_REQUIRE(n_tri == L->mesh_n_tri && n_vert == L->mesh_n_vert && n_mesh == L->mesh_n_mesh,
                  "n_tri, n_vert and n_mesh must be those of the system's mesh");
    PADNE_REQUIRE((n_tri == 0 || (power_out && eta_out && dual_eta_out && delta_out && omega_out)) && (n_vert == 0 || G_out), "null argument");
    PADNE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nt = (size_t)(n_tri > 0 ? n_tri : 1), nv = (size_t)(n_vert > 0 ? n_vert : 1), nm = (size_t)n_mesh, no = (size_t)n_obj;
    Scratch sc(ctx);
    GoalOut out;
    double *d_w = nullptr;
    int *d_bad = nullptr;
    PADNE_TRY(sc.alloc(&d_w, no * (size_t)n_cols));
    PADNE_TRY(sc.alloc(&out.power, nt));
    PADNE_TRY(sc.alloc(&out.G0, 2 * nv));
    PADNE_TRY(sc.alloc(&out.eta0, nt));
    PADNE_TRY(sc.alloc(&out.mesh_E, nm));
    PADNE_TRY(sc.alloc(&out.mesh_P, nm));
    PADNE_TRY(sc.alloc(&out.mesh_max, nm));
    PADNE_TRY(sc.alloc(&out.mesh_face, nm));
    PADNE_TRY(sc.alloc(&out.eta, no * nt));
    PADNE_TRY(sc.alloc(&out.delta, no * nt));
    PADNE_TRY(sc.alloc(&out.omega, no * nt));
    PADNE_TRY(sc.alloc(&out.obj_omega, no * nm));
    PADNE_TRY(sc.alloc(&out.obj_delta, no * nm));
    PADNE_TRY(sc.alloc(&out.obj_top, no * nm));
    PADNE_TRY(sc.alloc(&out.obj_face, no * nm));
    PADNE_HIP_CHECK(hipMemcpyAsync(d_w, weights, sizeof(double) * no * (size_t)n_cols, hipMemcpyHostToDevice, s));
    PADNE_TRY(bad_flag_alloc(sc, s, &d_bad));
    PADNE_TRY(csr_goal_error(ctx, L, &k->err_vptr, &k->err_vface, n_cols, n_obj, d_w, k->v_final, out, d_bad));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_error_out, out.mesh_E, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_power_out, out.mesh_P, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_max_out, out.mesh_max, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_face_out, out.mesh_face, sizeof(long long) * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_omega_out, out.obj_omega, sizeof(double) * no * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_delta_out, out.obj_delta, sizeof(double) * no * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_top_out, out.obj_top, sizeof(double) * no * nm, hipMemcpyDeviceToHost, s));
    PADNE_HIP_CHECK(hipMemcpyAsync(mesh_top_face_out, out.obj_face, sizeof(long long) * no * nm, hipMemcpyDeviceToHost, s));
    PADNE_TRY(bad_flag_check(s, d_bad));
    if (n_vert > 0) PADNE_TRY(parallel_copy(k, G_out, out.G0, sizeof(double) * 2 * (size_t)n_vert, hipMemcpyDeviceToHost));
    if (n_tri > 0) {
        PADNE_TRY(parallel_copy(k, power_out, out.power, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, eta_out, out.eta0, sizeof(double) * (size_t)n_tri, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, dual_eta_out, out.eta, sizeof(double) * no * (size_t)n_tri, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, delta_out, out.delta, sizeof(double) * no * (size_t)n_tri, hipMemcpyDeviceToHost));
        PADNE_TRY(parallel_copy(k, omega_out, out.omega, sizeof(double) * no * (size_t)n_tri, hipMemcpyDeviceToHost));
    }
    return PADNE_OK;
}

// ---- test entry: one device array of the plan, as it lies there (include/padne_hip_probe.h) ----------------------------
extern "C" int padne_test_kkt_state(const padne_kkt *k, int32_t which, void *out_host, int64_t n_bytes) {
    PADNE_REQUIRE(k && k->ctx, "null argument");
    const bool ran = k->solved || k->finished;            // a stage 1 has completed: its columns are the plan's
    const long long N = k->N, nf = k->n_free, width = kkt_block_width(k->n_cols), n_rhs = k->n_cols + k->n_extra;
    const void *src = nullptr;
    long long bytes = 0;
    switch (which) {
    case PADNE_TEST_KKT_IMAP: src = k->imap; bytes = (long long)sizeof(int32_t) * N; break;
    case PADNE_TEST_KKT_SRC_OF: src = k->src_of; bytes = (long long)sizeof(int32_t) * nf; break;
    case PADNE_TEST_KKT_B: src = ran ? k->b : nullptr; bytes = (long long)sizeof(double) * n_rhs * nf; break;
    case PADNE_TEST_KKT_Y: src = ran ? k->y : nullptr; bytes = (long long)sizeof(double) * n_rhs * nf; break;
    case PADNE_TEST_KKT_C:
        // (stage 2 writes the caller's layout into c when it differs from the products' one: kkt_finish_block, same_layout)
        src = ran && k->has_c && !(k->finished && !(width == k->n_cols && k->n_cols <= 8)) ? k->c : nullptr;
        bytes = (long long)sizeof(double) * N * width;
        break;
    case PADNE_TEST_KKT_V: src = ran ? k->v : nullptr; bytes = (long long)sizeof(double) * N * width; break;
    case PADNE_TEST_KKT_Z: src = ran ? k->Z : nullptr; bytes = (long long)sizeof(double) * k->n_extra * N; break;
    default: break;
    }
    if (which == PADNE_TEST_KKT_Z && ran && k->n_extra == 0) src = k->v;      // (an empty array: any address serves)
    PADNE_REQUIRE(which >= PADNE_TEST_KKT_IMAP && which <= PADNE_TEST_KKT_Z, "unknown array");
    PADNE_REQUIRE(src != nullptr, "the plan does not hold this array (yet)");
    PADNE_REQUIRE(n_bytes == bytes && (bytes == 0 || out_host != nullptr), "byte count of the array");
    PADNE_HIP_CHECK(hipSetDevice(k->ctx->device));
    PADNE_HIP_CHECK(hipStreamSynchronize(k->ctx->stream));
    if (bytes > 0) PADNE_HIP_CHECK(hipMemcpy(out_host, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return PADNE_OK;
}
