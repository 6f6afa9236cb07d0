// The cubic B-spline free-form deformation of the augmentation operators (augment.hip): ONE expression for the basis and
// for the tensor-product sum, so that the fused kernel and pulpo_bspline_field form the same elastic displacement bit for bit - as
// affine_core.h does for the affine position.  A control lattice phi of integer spacing s voxels: voxel z lies in cell i = z / s at
// u = (z - i s) / s, and e(z) = sum_l B_l(u) phi[i + l], l = 0..3 (phi_j = a s (j - 1) reproduces e = a z).  fp32, fixed operation order, explicit
// fused multiply-adds: the compiler's contraction has nothing left to decide.
#pragma once
#include <hip/hip_runtime.h>

namespace pulpo {

// cell and the four basis values of voxel coordinate v >= 0 on a lattice of spacing s >= 2; one = true: a depth-1 axis, which has no
// B-spline factor (weight 1 on the axis' single node)
__device__ __forceinline__ int bspline_weights(int v, int s, bool one, float w[4]) {
    if (one) {
        w[0] = 1.f; w[1] = 0.f; w[2] = 0.f; w[3] = 0.f;
        return 0;
    }
    const int i = v / s;
    const float u = (float)(v - i * s) / (float)s;               // exact numerator; one correctly rounded division
    const float u2 = u * u, u3 = u2 * u, m = 1.f - u;
    const float sixth = 1.f / 6.f;
    w[0] = (m * m) * m * sixth;
    w[1] = __fmaf_rn(3.f, u3, __fmaf_rn(-6.f, u2, 4.f)) * sixth;
    w[2] = __fmaf_rn(-3.f, u3, __fmaf_rn(3.f, u2, __fmaf_rn(3.f, u, 1.f))) * sixth;
    w[3] = u3 * sixth;
    return i;
}

// sum_l sum_m wzy[4 l + m] * node[l * sz + m * sy]: the (z, y) part of the tensor product at one x node, l outer, m inner
__device__ __forceinline__ float bspline_column(const float* __restrict__ node, int sz, int sy, const float wzy[16]) {
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc = __fmaf_rn(wzy[4 * l + m], node[l * sz + m * sy], acc);
    return acc;
}

// sum_n wx[n] * col[n]: the x part
__device__ __forceinline__ float bspline_row(const float wx[4], const float* col) {
    return __fmaf_rn(wx[3], col[3], __fmaf_rn(wx[2], col[2], __fmaf_rn(wx[1], col[1], wx[0] * col[0])));
}

}  // namespace pulpo
