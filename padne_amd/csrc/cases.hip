// Element cases: the potentials of every case as a sparse combination of the columns of a solved block.
//
//   launch_combine_block : V'[i][c] = sum over the entries e of row c of a CSR weight matrix, in order, of
//                          w_val[e] * V[i][w_col[e]]                                  (padne_kkt_combine_block)
//
// A tall, skinny product bound by memory: V [N][n_cols] is read once and V' [N][n_out] written once.  A workgroup stages
// as many whole rows of V as fit kCombineTileDoubles (at least one: a row has at most 4096 columns) -- they are one
// contiguous run of V, read coalesced -- and its lanes then run over the (row, case) pairs of the tile, so that the
// stores of a row are contiguous in the case index.  The weights are staged in LDS next to the rows when they fit
// kCombineWeightBytes (an N-1 sweep over hundreds of resistors does: two entries per case); a larger weight matrix is read
// through the caches.  No atomics, a fixed order of every sum: two calls give the same bits.
//
// This file is compiled with -ffp-contract=off: the first product starts the sum and every further one is rounded before
// it is added, so a row of one entry with coefficient 1.0 copies the column's bits.
#include "common.hpp"

namespace padne {

constexpr int kCombineTileDoubles = 2048;         // 16 KiB of rows per workgroup when a row is no longer than that
constexpr int kCombineWeightBytes = 24 * 1024;    // weights (row pointer, columns, values) staged in LDS up to this size

// rows of V a workgroup stages at a time
static inline int combine_tile_rows(int n_cols) { return n_cols >= kCombineTileDoubles ? 1 : kCombineTileDoubles / n_cols; }

// LDS of the staged weights: values first (8-byte aligned), then the columns and the row pointer
static inline size_t combine_weight_bytes(int n_out, long long nnz) {
    return sizeof(double) * (size_t)nnz + sizeof(int) * (size_t)nnz + sizeof(int) * ((size_t)n_out + 1);
}

template <bool kStageWeights>
__global__ __launch_bounds__(256) void combine_block_kernel(const long long N, const int n_cols, const int n_out, const int tile_rows,
                                                            const int nnz, const int *__restrict__ w_ptr,
                                                            const int *__restrict__ w_col, const double *__restrict__ w_val,
                                                            const double *__restrict__ V, double *__restrict__ out) {
    extern __shared__ double combine_lds[];
    double *rows = combine_lds;                                        // [tile_rows][n_cols]
    const long long i0 = (long long)blockIdx.x * tile_rows;
    if (i0 >= N) return;
    const int n_rows = (int)(N - i0 < tile_rows ? N - i0 : tile_rows);
    const int n_stage = n_rows * n_cols;                               // <= max(kCombineTileDoubles, 4096)
    const double *src = V + i0 * n_cols;
    for (int t = threadIdx.x; t < n_stage; t += 256) rows[t] = src[t];
    const int *ptr = w_ptr, *col = w_col;
    const double *val = w_val;
    if (kStageWeights) {
        double *s_val = combine_lds + (size_t)tile_rows * n_cols;
        int *s_col = (int *)(s_val + nnz);
        int *s_ptr = s_col + nnz;
        for (int e = threadIdx.x; e < nnz; e += 256) {
            s_val[e] = w_val[e];
            s_col[e] = w_col[e];
        }
        for (int c = threadIdx.x; c <= n_out; c += 256) s_ptr[c] = w_ptr[c];
        ptr = s_ptr;
        col = s_col;
        val = s_val;
    }
    __syncthreads();
    double *dst = out + i0 * n_out;
    const int n_pairs = n_rows * n_out;                                // <= 2048 * 4096
    for (int p = threadIdx.x; p < n_pairs; p += 256) {
        const int row = p / n_out;
        const int c = p - row * n_out;
        const double *v = rows + (size_t)row * n_cols;
        const int lo = ptr[c], hi = ptr[c + 1];
        double acc = 0.0;
        if (lo < hi) {
            acc = val[lo] * v[col[lo]];
            for (int e = lo + 1; e < hi; ++e) acc = acc + val[e] * v[col[e]];
        }
        dst[p] = acc;
    }
}

// V_dev [N][n_cols] -> out_dev [N][n_out] by the CSR weights on the device (w_ptr_dev [n_out + 1] with w_ptr[n_out] = nnz,
// columns checked by the caller to lie in [0, n_cols)).  Asynchronous on the context's stream.
int launch_combine_block(padne_ctx *ctx, long long N, int n_cols, int n_out, long long nnz, const int *w_ptr_dev,
                         const int *w_col_dev, const double *w_val_dev, const double *V_dev, double *out_dev) {
    PADNE_REQUIRE(N >= 0 && n_cols >= 1 && n_cols <= 4096 && n_out >= 1 && n_out <= 4096, "block shape");
    PADNE_REQUIRE(nnz >= 0 && nnz <= (long long)n_cols * n_out, "number of weights");
    if (N == 0) return PADNE_OK;
    const int tile_rows = combine_tile_rows(n_cols);
    const long long n_blocks = (N + tile_rows - 1) / tile_rows;
    PADNE_REQUIRE(n_blocks <= 0x7fffffffLL, "too many rows for one launch");
    const size_t row_bytes = sizeof(double) * (size_t)tile_rows * (size_t)n_cols;
    const size_t weight_bytes = combine_weight_bytes(n_out, nnz);
    const bool stage = weight_bytes <= (size_t)kCombineWeightBytes;
    if (stage)
        hipLaunchKernelGGL(combine_block_kernel<true>, dim3((unsigned)n_blocks), dim3(256), row_bytes + weight_bytes, ctx->stream,
                           N, n_cols, n_out, tile_rows, (int)nnz, w_ptr_dev, w_col_dev, w_val_dev, V_dev, out_dev);
    else
        hipLaunchKernelGGL(combine_block_kernel<false>, dim3((unsigned)n_blocks), dim3(256), row_bytes, ctx->stream, N, n_cols,
                           n_out, tile_rows, (int)nnz, w_ptr_dev, w_col_dev, w_val_dev, V_dev, out_dev);
    PADNE_HIP_CHECK(hipGetLastError());
    return PADNE_OK;
}

}  // namespace padne
