// The affine transform of the pre-alignment operators (affine.hip): ONE expression for the position an affine map
// sends a voxel to and for the displacement it stands for, so that every kernel that forms them agrees bit for bit - as sampling.h does
// for the sample coordinate.  theta = [M | t] (3 x 4, row-major) in voxel units of a grid (D, H, W), about the grid's centre
// c = ((D-1)/2, (H-1)/2, (W-1)/2):  p = c + M (v - c) + t,  d = p - v (SpatialTransformer's convention: warp3d(d, img) samples img at
// sample_coord(v, d(v), Sg, Si)).  fp32, fixed operation order: the three products are explicit fused multiply-adds, innermost x, so
// the compiler's contraction has nothing left to decide.  The identity [I | 0] gives d = 0 exactly (v - c and c + (v - c) are exact).
#pragma once
#include <hip/hip_runtime.h>

namespace pulpo {

struct Affine {
    float m[12];      // theta of one batch element, row-major [a][b]: m[4 a + b], b = 3 the translation
    float cz, cy, cx; // the centre of the frame's grid
};

// wave-uniform: every thread of a block reads the same twelve values (scalar loads)
__device__ __forceinline__ Affine affine_load(const float* __restrict__ theta, int D, int H, int W) {
    Affine A;
#pragma unroll
    for (int k = 0; k < 12; ++k) A.m[k] = theta[k];
    A.cz = 0.5f * (float)(D - 1);
    A.cy = 0.5f * (float)(H - 1);
    A.cx = 0.5f * (float)(W - 1);
    return A;
}

// row a of M (v - c) + t, with u = v - c
__device__ __forceinline__ float affine_row(const float* __restrict__ r, float uz, float uy, float ux) {
    return __fmaf_rn(r[0], uz, __fmaf_rn(r[1], uy, __fmaf_rn(r[2], ux, r[3])));
}

// p = c + M (v - c) + t at the (possibly fractional) position (z, y, x) of the frame's grid
__device__ __forceinline__ void affine_pos(const Affine& A, float z, float y, float x, float p[3]) {
    const float uz = z - A.cz, uy = y - A.cy, ux = x - A.cx;
    p[0] = A.cz + affine_row(A.m, uz, uy, ux);
    p[1] = A.cy + affine_row(A.m + 4, uz, uy, ux);
    p[2] = A.cx + affine_row(A.m + 8, uz, uy, ux);
}

// d = p - v
__device__ __forceinline__ void affine_disp(const Affine& A, float z, float y, float x, float d[3]) {
    float p[3];
    affine_pos(A, z, y, x, p);
    d[0] = p[0] - z;
    d[1] = p[1] - y;
    d[2] = p[2] - x;
}

}  // namespace pulpo
