// Per-face arithmetic shared by the assembly (assemble.hip), the face kernels (fields.hip) and the field sampler
// (sample.hip).  Every translation unit that includes this is compiled with -ffp-contract=off: the expressions round
// exactly as written, which is what lets a numpy restatement reproduce their bits.
#pragma once

#include <hip/hip_runtime.h>

namespace padne {

__device__ __forceinline__ int find_segment(const long long *__restrict__ offs, int n_seg, long long i) {
    // largest m with offs[m] <= i   (offs has n_seg+1 entries, offs[0] = 0)
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// |cot(theta_o)| / 2 for the edge (i,k) seen from the opposite corner o   -- mesh.py:136-138
__device__ __forceinline__ double cot_half(double ix, double iy, double kx, double ky, double ox, double oy) {
    const double vix = ix - ox, viy = iy - oy;
    const double vkx = kx - ox, vky = ky - oy;
    const double dot = vix * vkx + viy * vky;
    const double cross = vix * vky - viy * vkx;
    return fabs(dot / cross) / 2;
}

// ---- power density ---------------------------------------------------------------------------
// compute_triangle_gradient (solver.py:689-725) with the face vertex order of the reference:
// Face.edge is the last interior half-edge created (v3->v1, mesh.py:320-325) so face.vertices
// yields (v3, v1, v2).
__device__ __forceinline__ double interp(double x1, double y1, double x2, double y2, double x3, double y3,
                                         double f1, double f2, double f3, double x, double y) {
    const double D = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3);
    const double l1 = ((y2 - y3) * (x - x3) + (x3 - x2) * (y - y3)) / D;
    const double l2 = ((y3 - y1) * (x - x3) + (x1 - x3) * (y - y3)) / D;
    const double l3 = 1 - l1 - l2;
    return l1 * f1 + l2 * f2 + l3 * f3;
}

// the face gradient and sigma |grad V|^2 of compute_power_density (solver.py:728-745), shared by every form of the kernel
__device__ __forceinline__ void face_gradient_of(double x1, double y1, double x2, double y2, double x3, double y3, double f1,
                                                 double f2, double f3, double &gx, double &gy) {
    gx = interp(x1, y1, x2, y2, x3, y3, f1, f2, f3, x1 + 1, y1) - f1;
    gy = interp(x1, y1, x2, y2, x3, y3, f1, f2, f3, x1, y1 + 1) - f1;
}

__device__ __forceinline__ double face_power_of(double gx, double gy, double s) {
    const double jx = gx * s, jy = gy * s;      // J = E * conductivity
    return jx * gx + jy * gy;                   // J.dot(E)
}

// The power of a face in the weights' form, sigma sum_{edges (i,k)} w_ik (f_i - f_k)^2 with w_ik = cot_half of the corner
// opposite the edge: what the assembly's rows dissipate, so the faces' sum balances the elements' powers (Tellegen).  Shared
// by the per-mesh power of current_cases_face_kernel (fields.hip) and the heat load of thermal.hip: both round alike
__device__ __forceinline__ double face_edge_power(double s, double w12, double w23, double w31, double f1, double f2, double f3) {
    const double d12 = f1 - f2, d23 = f2 - f3, d31 = f3 - f1;
    return s * ((w12 * d12 * d12 + w23 * d23 * d23) + w31 * d31 * d31);
}

// orient(a, b, p) > 0: p lies left of a -> b.  Evaluated exactly so (the library builds with -ffp-contract=off), which
// lets a numpy restatement reproduce every decision of the cut rule and of the sampler's owner rule
__device__ __forceinline__ double orient(double ax, double ay, double bx, double by, double px, double py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

}  // namespace padne
