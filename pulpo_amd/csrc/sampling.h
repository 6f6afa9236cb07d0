// Arithmetic shared by the kernels that must agree bit for bit: the grid_sample coordinate of the deformable warp (warp.hip, labels.hip,
// inverse.hip), the squaring step of the forward integrations (warp.hip, inverse.hip) and the Welford step of the Monte-Carlo moments
// (uncertainty.hip, labels.hip).  One definition, so one expression.  Also the geometric sampler of the inverse-field operators (inverse.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pulpo {

struct Corner {
    int i0, i1;
    float f;       // fraction towards i1
    float dscale;  // d(coord)/d(displacement); 0 where the coordinate was clamped
};

__device__ __forceinline__ Corner sample_coord(float pos, float disp, int Sg, int Si) {
    if (Sg == 1) {            // a depth-1 grid is the reference's 2-D case (bilinear grid_sample over H, W): no coordinate along this axis
        Corner r;
        r.i0 = 0; r.i1 = 0; r.f = 0.f; r.dscale = 0.f;
        return r;
    }
    float t = pos + disp;
    t = t / (float)(Sg - 1);
    t = t - 0.5f;
    t = 2.f * t;
    float c = ((t + 1.f) * (float)Si - 1.f) / 2.f;
    Corner r;
    const float hi = (float)(Si - 1);
    r.dscale = (c > 0.f && c < hi) ? (float)Si / (float)(Sg - 1) : 0.f;   // ATen clip_coordinates_set_grad
    c = fminf(hi, fmaxf(c, 0.f));
    const float fl = floorf(c);
    r.i0 = (int)fl;
    r.i1 = min(r.i0 + 1, Si - 1);
    r.f = c - fl;
    return r;
}

// One scaling-and-squaring step of VecInt (network_blocks.py:173-177: v <- v + warp(v, v)) at voxel vox = (z, y, x): the 3-channel field
// fld ([3][V] planar, in LDS or in memory) is image and displacement at once.  nv[c] = fld_c[vox] + trilinear(fld_c, vox displaced by
// fld[:, vox]).  The one gather of the forward integrations (warp.hip's one-launch kernel, inverse.hip's pair kernels); the expression is
// the one warp_fwd_kernel<3> evaluates with add = img = df.
__device__ __forceinline__ void vecint_step_voxel(const float* fld, int V, int vox, int D, int H, int W, float nv[3]) {
    const int x = vox % W, y = (vox / W) % H, z = vox / (W * H);
    const float* f1 = fld + (long)V;
    const float* f2 = f1 + (long)V;
    const Corner cz = sample_coord((float)z, fld[vox], D, D);
    const Corner cy = sample_coord((float)y, f1[vox], H, H);
    const Corner cx = sample_coord((float)x, f2[vox], W, W);
    const int o00 = (cz.i0 * H + cy.i0) * W, o01 = (cz.i0 * H + cy.i1) * W;
    const int o10 = (cz.i1 * H + cy.i0) * W, o11 = (cz.i1 * H + cy.i1) * W;
    const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* s = c == 0 ? fld : (c == 1 ? f1 : f2);
        float val = wz0 * wy0 * wx0 * s[o00 + cx.i0] + wz0 * wy0 * cx.f * s[o00 + cx.i1] + wz0 * cy.f * wx0 * s[o01 + cx.i0] +
                    wz0 * cy.f * cx.f * s[o01 + cx.i1] + cz.f * wy0 * wx0 * s[o10 + cx.i0] + cz.f * wy0 * cx.f * s[o10 + cx.i1] +
                    cz.f * cy.f * wx0 * s[o11 + cx.i0] + cz.f * cy.f * cx.f * s[o11 + cx.i1];
        val += s[vox];
        nv[c] = val;
    }
}

// The geometric sampler of the inverse-field operators (inverse.hip): position p + d in VOXEL units, clamped to [0, S - 1], upper corner
// min(i0 + 1, S - 1) - so a zero field is the identity.  Not sample_coord: that one is the reference SpatialTransformer's (S-1)-normalised,
// align_corners=False coordinate.  In double: the residual d_b + d_a(p + d_b) cancels to a few percent of the displacements it is made of.
struct GeoCorner {
    int i0, i1;
    double f;      // fraction towards i1
};

__device__ __forceinline__ GeoCorner geo_coord(double pos, int S) {
    const double c = fmin((double)(S - 1), fmax(pos, 0.0));           // (fmax(NaN, 0) = 0: the index stays inside the field whatever the input)
    const double fl = floor(c);
    GeoCorner r;
    r.i0 = (int)fl;
    r.i1 = min(r.i0 + 1, S - 1);
    r.f = c - fl;
    return r;
}

// trilinear value of one channel plane s ([D][H][W]) at the corners / fractions of (cz, cy, cx)
__device__ __forceinline__ double geo_sample(const float* __restrict__ s, const GeoCorner& cz, const GeoCorner& cy, const GeoCorner& cx, int H, int W) {
    const long o00 = ((long)cz.i0 * H + cy.i0) * W, o01 = ((long)cz.i0 * H + cy.i1) * W;
    const long o10 = ((long)cz.i1 * H + cy.i0) * W, o11 = ((long)cz.i1 * H + cy.i1) * W;
    const double x0 = 1.0 - cx.f, x1 = cx.f;
    const double r00 = x0 * (double)s[o00 + cx.i0] + x1 * (double)s[o00 + cx.i1], r01 = x0 * (double)s[o01 + cx.i0] + x1 * (double)s[o01 + cx.i1];
    const double r10 = x0 * (double)s[o10 + cx.i0] + x1 * (double)s[o10 + cx.i1], r11 = x0 * (double)s[o11 + cx.i0] + x1 * (double)s[o11 + cx.i1];
    const double q0 = (1.0 - cy.f) * r00 + cy.f * r01, q1 = (1.0 - cy.f) * r10 + cy.f * r11;
    return (1.0 - cz.f) * q0 + cz.f * q1;
}

// Fold sample x into the running (mean, M2) of one element; k = number of samples including this one, inv = 1 / k
__device__ __forceinline__ void welford_step(float x, float& mean, float& m2, int k, float inv) {
    if (k == 1) {
        mean = x;
        m2 = 0.f;
    } else {
        const float mu = mean;
        const float d = x - mu;
        const float mu2 = mu + d * inv;
        mean = mu2;
        m2 += d * (x - mu2);
    }
}

}  // namespace pulpo
