// The cubic B-spline interpolator of the final resample (cubic.hip): ONE expression for the basis, for its derivative,
// for the whole-sample mirror index and for the start values of the recursive prefilter, each used by every kernel that needs it - as
// sampling.h does for the sample coordinate (which these kernels take from there unchanged) and bspline_core.h for the augmentation lattice.
// fp32, fixed operation order, explicit fused multiply-adds: the compiler's contraction has nothing left to decide.
#pragma once
#include <hip/hip_runtime.h>

namespace pulpo {

// Unser's recursive filter of the cubic B-spline: one pole z = sqrt(3) - 2 and a gain of (1 - z)(1 - 1/z) = 6 per axis
constexpr float kCubicPole = -0.26794919243112270647f;
constexpr float kCubicInvPole = -3.73205080756887729353f;
constexpr float kCubicGain = 6.f;
// |z|^32 = 5e-19, twelve orders below fp32 resolution: on a line longer than this the causal start sum stops here (and the mirrored terms,
// all below |z|^32, are dropped); a shorter line takes the exact closed form
constexpr int kCubicHorizon = 32;

// whole-sample mirror of tap j into an axis of N samples (period 2 (N - 1): m(-1) = 1, m(N) = N - 2); valid for -1 <= j <= N + 1, which is
// every tap i - 1 .. i + 2 of a cell 0 <= i <= N - 1.  An axis of one sample has one index.
__device__ __forceinline__ int cubic_mirror(int j, int N) {
    if (N == 1) return 0;
    const int p = 2 * (N - 1);
    j = j < 0 ? -j : j;
    if (j >= p) j -= p;
    return j < N ? j : p - j;
}

// B_0..B_3 at fraction f: the polynomials of bspline_weights; one = true: an axis without a coordinate (weight 1 on the first tap)
__device__ __forceinline__ void cubic_weights(float f, bool one, float w[4]) {
    if (one) {
        w[0] = 1.f; w[1] = 0.f; w[2] = 0.f; w[3] = 0.f;
        return;
    }
    const float f2 = f * f, f3 = f2 * f, m = 1.f - f;
    const float sixth = 1.f / 6.f;
    w[0] = (m * m) * m * sixth;
    w[1] = __fmaf_rn(3.f, f3, __fmaf_rn(-6.f, f2, 4.f)) * sixth;
    w[2] = __fmaf_rn(-3.f, f3, __fmaf_rn(3.f, f2, __fmaf_rn(3.f, f, 1.f))) * sixth;
    w[3] = f3 * sixth;
}

// B'_0..B'_3 at fraction f (they sum to zero); an axis without a coordinate has no derivative
__device__ __forceinline__ void cubic_dweights(float f, bool one, float d[4]) {
    if (one) {
        d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f;
        return;
    }
    const float f2 = f * f, m = 1.f - f;
    d[0] = -0.5f * (m * m);
    d[1] = 0.5f * __fmaf_rn(3.f, f2, -4.f * f);
    d[2] = 0.5f * __fmaf_rn(-3.f, f2, __fmaf_rn(2.f, f, 1.f));
    d[3] = 0.5f * f2;
}

// the four mirrored tap indices of cell i (taps i - 1 .. i + 2) on an axis of N samples; one = true: the single tap 0
__device__ __forceinline__ void cubic_taps(int i, int N, bool one, int t[4]) {
#pragma unroll
    for (int l = 0; l < 4; ++l) t[l] = one ? 0 : cubic_mirror(i - 1 + l, N);
}

// Causal start c+[0] of a line of N >= 2 samples s(k) (already multiplied by the gain):
//   (s[0] + z^(N-1) s[N-1] + sum_{k=1..N-2} (z^k + z^(2N-2-k)) s[k]) / (1 - z^(2N-2)),
// exact for N <= kCubicHorizon, the first kCubicHorizon terms of sum z^k s[k] beyond.  s(k) is read for k < min(N, kCubicHorizon) only.
template <class Load>
__device__ __forceinline__ float cubic_causal_start(Load s, int N) {
    const float z = kCubicPole;
    if (N > kCubicHorizon) {
        float acc = s(0), zk = z;
        for (int k = 1; k < kCubicHorizon; ++k) {
            acc = __fmaf_rn(zk, s(k), acc);
            zk *= z;
        }
        return acc;
    }
    float zn = 1.f;
    for (int k = 1; k < N; ++k) zn *= z;                       // z^(N-1)
    const float z2n = zn * zn;                                  // z^(2N-2)
    float acc = __fmaf_rn(zn, s(N - 1), s(0));
    float zk = z, zr = z2n * kCubicInvPole;                     // z^k and z^(2N-2-k)
    for (int k = 1; k < N - 1; ++k) {
        acc = __fmaf_rn(zk + zr, s(k), acc);
        zk *= z;
        zr *= kCubicInvPole;
    }
    return acc / (1.f - z2n);
}

// anticausal start c[N-1] from the last two causal values
__device__ __forceinline__ float cubic_anticausal_start(float cp_last, float cp_before) {
    const float z = kCubicPole;
    return (z / (z * z - 1.f)) * __fmaf_rn(z, cp_before, cp_last);
}

}  // namespace pulpo
