// Arithmetic shared by the kernels that must agree bit for bit: the grid_sample coordinate of the deformable warp (warp.hip, labels.hip)
// and the Welford step of the Monte-Carlo moments (uncertainty.hip, labels.hip).  One definition, so one expression and one contraction.
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
