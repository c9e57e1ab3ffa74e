// Point location over the meshes of a layer, as the translation units that use it see it: the field sampler (sample.hip),
// which owns the index build, and the inter-layer coupling (stack.hip), which asks for the owner of every vertex of one
// layer among the faces of another.  The owner rule is stated at the top of sample.hip; both units are compiled with
// -ffp-contract=off, so the sides written once here round the same way in both.
#pragma once

#include "common.hpp"
#include "face.hpp"

#include <vector>

namespace padne {

constexpr int kListBound = 16;                    // list entries per face of a layer at the most; beyond it the grid is coarsened
constexpr int kMaxBinsPerSide = 32768;

// the grid of one layer: bin (bx, by) is number bin0 + by * nbx + bx of the index's bins
struct LayerGrid {
    double x0 = 0, y0 = 0, sx = 0, sy = 0;        // lower corner of the layer's bounding box, bins per mm
    int nbx = 1, nby = 1;
    long long bin0 = 0;
};

// the bin of a coordinate: monotone in x (a difference, a product with a positive constant, floor and a clamp are), so a
// point between the ends of an interval falls into a bin between the bins of the ends -- also beyond the bounding box
__device__ __forceinline__ int bin_of(double x, double x0, double s, int n) {
    if (n == 1) return 0;
    double t = floor((x - x0) * s);
    t = fmin(fmax(t, 0.0), (double)(n - 1));
    return (int)t;
}

// side of q of the edge (i, k) as the face runs it (the owner rule)
__device__ __forceinline__ double edge_side(int gi, int gk, double xi, double yi, double xk, double yk, double qx, double qy) {
    return gi < gk ? orient(xi, yi, xk, yk, qx, qy) : -orient(xk, yk, xi, yi, qx, qy);
}

// The owner of q among the faces of the layer with grid g: the candidates of q's bin, the containing one with the lowest
// global index; 0x7fffffff for none.  wa, wb, wc: the owner's sides o_a, o_b, o_c (the edges opposite its corners tri[0],
// tri[1], tri[2]); n_tested: the candidates looked at
constexpr int kNoOwner = 0x7fffffff;
__device__ __forceinline__ int locate_owner(const LayerGrid &g, const int *__restrict__ bin_off, const int *__restrict__ bin_face,
                                            const int *__restrict__ gtri, const double *__restrict__ xy, double qx, double qy,
                                            double &wa, double &wb, double &wc, unsigned long long &n_tested) {
    const long long bin = g.bin0 + (long long)bin_of(qy, g.y0, g.sy, g.nby) * g.nbx + bin_of(qx, g.x0, g.sx, g.nbx);
    const int lo = bin_off[bin], hi = bin_off[bin + 1];
    n_tested = (unsigned long long)(hi - lo);
    int owner = kNoOwner;
    wa = wb = wc = 0.0;
    for (int e = lo; e < hi; ++e) {
        const int f = bin_face[e];
        const int a = gtri[3 * (long long)f], b = gtri[3 * (long long)f + 1], c = gtri[3 * (long long)f + 2];
        const double xa = xy[2 * (long long)a], ya = xy[2 * (long long)a + 1];
        const double xb = xy[2 * (long long)b], yb = xy[2 * (long long)b + 1];
        const double xc = xy[2 * (long long)c], yc = xy[2 * (long long)c + 1];
        const double oa = edge_side(b, c, xb, yb, xc, yc, qx, qy);
        const double ob = edge_side(c, a, xc, yc, xa, ya, qx, qy);
        const double oc = edge_side(a, b, xa, ya, xb, yb, qx, qy);
        const bool in = ((oa >= 0.0 && ob >= 0.0 && oc >= 0.0) || (oa <= 0.0 && ob <= 0.0 && oc <= 0.0)) &&
                        !(oa == 0.0 && ob == 0.0 && oc == 0.0);
        if (in && f < owner) {
            owner = f;
            wa = oa;
            wb = ob;
            wc = oc;
        }
    }
    return owner;
}

// sample.hip.  locate_global_corners: gtri[f] = mesh_voff[m] + tri[f] for every face, queued on the stream; *err_dev (a
// zeroed device int) is set for a triangle index out of range.  locate_build_bins: the index over the faces gtri -- per
// layer (mesh_layer[m]; negative: the mesh is left out) the grid of its bounding box lo / hi[n_layer][2] (bins_hint bins, 0:
// half a bin per face), then count, scan, fill, coarsened while a layer's lists are longer than kListBound entries per face.  *bin_off and *bin_face are pool
// allocations the caller owns (also after an error, where they may be set); all other arrays are the caller's, on the
// device but for lo, hi and layer_faces.  Returns with the stream drained.
int locate_global_corners(padne_ctx *ctx, long long n_tri, const int *tri, int n_mesh, const long long *mesh_voff,
                          const long long *mesh_toff, int *gtri, int *err_dev);
int locate_build_bins(padne_ctx *ctx, int n_layer, const double *lo, const double *hi, int64_t bins_hint,
                      const std::vector<int64_t> &layer_faces, long long n_tri, const int *gtri, const double *xy, int n_mesh,
                      const long long *mesh_toff, const int *mesh_layer, std::vector<LayerGrid> &grid,
                      std::vector<int64_t> &layer_entries, int **bin_off, int **bin_face);

}  // namespace padne
