// Expressions shared by the BatchNorm / LeakyReLU passes (norm_act.hip), the 1x1x1 head kernels that form the activation and its gradient
// themselves (heads.hip: the last ConvUnit in front of a head - its output z and the gradient dz have one reader each and are never written)
// and the convolution kernels (conv3d*.hip): their eval-mode fused store is bn_lrelu, and the data-gradient kernels that deliver the
// BatchNorm-backward sums of the unit in front take bn_bwd_reduce_step per element.
// ONE definition each, as sampling.h does for the warp coordinate: the fp32 results of the fused kernels are then the separate passes' bits.
#pragma once
#include "common.h"

namespace pulpo {

// z = leaky_relu(y * scale + shift)
__device__ __forceinline__ float bn_lrelu(float y, float scale, float shift, float slope) {
    const float t = y * scale + shift;
    return t > 0.f ? t : t * slope;
}

// One element of the first BatchNorm-backward pass: dbn = dz * lrelu'(bn(y));  s0 += dbn,  s1 += dbn * (y - m32), m32 = the batch mean rounded
// to fp32.  All fp32: the difference of two floats carries a relative error of 2^-24 however close they are, and what the ROUNDED mean leaves
// out is added back, in double, by pulpo_bn_bwd_finalize:  sum dbn * xhat = rstd * (sum dbn * (y - m32) - (mean - m32) * sum dbn).
// (bn_lrelu_bwd_reduce_kernel, heads_bwd_kernel<.., BN> and the *_bnred data-gradient epilogues write partial rows the suite holds to the same bits)
__device__ __forceinline__ void bn_bwd_reduce_step(float dz, float y, float scale, float shift, float m32, float slope, float& s0, float& s1) {
    const float bn = y * scale + shift;
    const float d = bn > 0.f ? dz : dz * slope;
    s0 += d;
    s1 = fmaf(d, y - m32, s1);
}

// The six per-channel constants of the second BatchNorm-backward pass, kst = [6][C] in LDS: scale, shift, m32, B, C hi, C lo with
//   dy = scale * dbn + B * (y - m32) + C,   B = -scale * c2 * rstd,   C = -scale * (c1 + c2 * rstd * (m32 - mean))
// formed in double from the exact means (coef: the unit's coefficient block, totd: mean dbn | mean dbn * xhat); C keeps 48 bits as (hi, lo).
__device__ __forceinline__ void bn_bwd_constants(float* kst, const float* __restrict__ coef, const double* __restrict__ totd, int C) {
    for (int ch = threadIdx.x; ch < C; ch += blockDim.x) {
        const double* cd = reinterpret_cast<const double*>(coef + 4 * C);
        const float sc_ = coef[2 * C + ch], m32_ = coef[ch];
        const double mean = cd[ch], rstd = cd[C + ch], c1 = totd[ch], c2 = totd[C + ch];
        const double b = -(double)sc_ * c2 * rstd;
        const double cc = -(double)sc_ * (c1 + c2 * rstd * ((double)m32_ - mean));
        const float chi_ = (float)cc;
        kst[0 * C + ch] = sc_;
        kst[1 * C + ch] = coef[3 * C + ch];
        kst[2 * C + ch] = m32_;
        kst[3 * C + ch] = (float)b;
        kst[4 * C + ch] = chi_;
        kst[5 * C + ch] = (float)(cc - (double)chi_);
    }
}

// pre-activation gradients of the mu / sigma head from the 15 planar values of a voxel, sv = g0[3] | g1[3] | g2[3] | eps[3] | sigma[3]
// (gradients of mu, sigma, the sample; absent operands stored as 0):  dmu = g0 + g2 ; dsigma = g1 + g2 * eps ; softplus' = 1 - exp(-sigma)
__device__ __forceinline__ void head_dpre6(const float* sv, float (&dpre)[6]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gz = sv[6 + j];
        dpre[j] = sv[j] + gz;
        const float gs = sv[3 + j] + gz * sv[9 + j];
        dpre[3 + j] = gs * (1.f - expf(-sv[12 + j]));
    }
}

}  // namespace pulpo
