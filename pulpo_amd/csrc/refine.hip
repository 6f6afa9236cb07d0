// Anchored Adam over a flat arena of velocity fields: the parameter side of instance-specific refinement (pulpo_amd/refine.py, DESIGN.md
// section 3k).  One launch covers every level's field.  With an anchor (mean, optional per-element precision prec; a = prec ? prec[e] : 1,
// d = p[e] - mean[e]) the gradient used is g[e] + a d and the block's partial receives 0.5 a d^2 - the anchor's value at the iterate the
// forward pass saw, before the update; then adam_kernel's update (optim.hip).  Without an anchor the call is pulpo_adam_step's own launch.
// One streaming pass: up to 6 reads and 3 writes per element.  The sum within a block is ordered (wave shuffles, then four adds; no float
// atomics) and finished by pulpo_colsum in double: deterministic.
#include "common.h"

extern "C" int pulpo_loss_blocks(int64_t n);
extern "C" int pulpo_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps, int step,
                               float gscale, void* stream);

namespace {

// PREC: a per-element precision beside the mean.  partial (nullable) has nparts >= gridDim.x slots: block b writes its sum to slot b, the
// slots past the grid are cleared so that a column sum over all nparts is the anchor's value.
template <bool PREC>
__global__ __launch_bounds__(256) void anchored_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                              const float* __restrict__ mean, const float* __restrict__ prec, long n, float lr, float beta1,
                                                              float omb1, float beta2, float omb2, float eps, float bc1, float bc2_sqrt,
                                                              float* __restrict__ partial, int nparts) {
    __shared__ float sh[4];
    const long n4 = n >> 2;
    const float step = lr / bc1;
    float local = 0.f;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[e], gg = reinterpret_cast<const float4*>(g)[e];
        float4 mm = reinterpret_cast<float4*>(m)[e], vv = reinterpret_cast<float4*>(v)[e];
        float4 mu = reinterpret_cast<const float4*>(mean)[e], aa = make_float4(1.f, 1.f, 1.f, 1.f);
        if constexpr (PREC) aa = reinterpret_cast<const float4*>(prec)[e];
        float* pa = &pp.x; float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x; float* ua = &mu.x; float* ca = &aa.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = pa[k] - ua[k];
            const float ad = PREC ? ca[k] * d : d;
            const float gr = ga[k] + ad;
            local += 0.5f * ad * d;
            ma[k] = beta1 * ma[k] + omb1 * gr;
            va[k] = beta2 * va[k] + omb2 * gr * gr;
            pa[k] -= step * ma[k] / (sqrtf(va[k]) / bc2_sqrt + eps);
        }
        reinterpret_cast<float4*>(p)[e] = pp;
        reinterpret_cast<float4*>(m)[e] = mm;
        reinterpret_cast<float4*>(v)[e] = vv;
    }
    for (long e = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const float d = p[e] - mean[e];
        const float ad = PREC ? prec[e] * d : d;
        const float gr = g[e] + ad;
        local += 0.5f * ad * d;
        const float mn = beta1 * m[e] + omb1 * gr;
        const float vn = beta2 * v[e] + omb2 * gr * gr;
        m[e] = mn; v[e] = vn;
        p[e] -= step * mn / (sqrtf(vn) / bc2_sqrt + eps);
    }
    if (partial != nullptr) {                        // (uniform over the grid: no thread skips the block sum's barriers)
        const float t = pulpo::block_sum_256(local, sh);
        if (threadIdx.x == 0) {
            partial[blockIdx.x] = t;
            for (int s = blockIdx.x + gridDim.x; s < nparts; s += gridDim.x) partial[s] = 0.f;
        }
    }
}

}  // namespace

// step >= 1; beta1, beta2 as doubles and the bias corrections formed in double, as pulpo_adam_step.  mean == NULL: plain Adam - the call is
// pulpo_adam_step's launch with gscale = 1, hence bit-identical to it (partial is then left alone).  partial (nullable): pulpo_loss_blocks(n)
// floats, all of them written; finish with pulpo_colsum.  The grid is adam_step's (float4 groups / 256, at most 4096 blocks), and at most
// pulpo_loss_blocks(n) when partial is given: one slot per block.
PULPO_API int pulpo_anchored_adam_step(float* p, const float* g, float* m, float* v, const float* mean, const float* prec, int64_t n, float lr,
                                       double beta1, double beta2, float eps, int step, float* partial, void* stream) {
    PULPO_REQUIRE(p && g && m && v && n > 0 && step >= 1, "anchored_adam_step: bad arguments");
    PULPO_REQUIRE(mean || !prec, "anchored_adam_step: prec needs mean");
    PULPO_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)mean) | ((uintptr_t)prec) | ((uintptr_t)partial)) & 15) == 0,
                  "anchored_adam_step: arenas must be 16-byte aligned");
    if (!mean) return pulpo_adam_step(p, g, m, v, n, lr, beta1, beta2, eps, step, 1.f, stream);
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    int nblk = (int)std::max<long>(1, std::min<long>(((n >> 2) + 255) / 256, 4096));
    const int nparts = partial ? pulpo_loss_blocks(n) : 0;
    if (nparts) nblk = std::min(nblk, nparts);
    const float b1 = (float)beta1, o1 = (float)(1.0 - beta1), b2 = (float)beta2, o2 = (float)(1.0 - beta2), c1 = (float)bc1, c2 = (float)sqrt(bc2);
    hipStream_t st = (hipStream_t)stream;
    if (!prec)
        hipLaunchKernelGGL(anchored_adam_kernel<false>, dim3(nblk), dim3(256), 0, st, p, g, m, v, mean, prec, (long)n, lr, b1, o1, b2, o2, eps, c1, c2, partial, nparts);
    else
        hipLaunchKernelGGL(anchored_adam_kernel<true>, dim3(nblk), dim3(256), 0, st, p, g, m, v, mean, prec, (long)n, lr, b1, o1, b2, o2, eps, c1, c2, partial, nparts);
    return pulpo::check_launch("anchored_adam_step");
}
