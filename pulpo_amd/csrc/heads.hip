// 1x1x1 channel-mixing heads C -> 3 (or C -> 3+3):
//   MuSigmaBlock + gauss_sampler  (reference: src/network_blocks.py:49-60, :7-8):  mu = Wm h + bm ;
//        sigma = softplus(Ws h + bs) ; z = mu + sigma * eps
//   VelocityField's last layer    (reference: src/network_blocks.py:81):           v = W h + b
// Input h is channels-last [pixel][C]; outputs are planar (B, 3, D*H*W) like the reference's tensors.
// HBM-bound (reads C floats, writes 3-9 per voxel): 8 lanes share one voxel, each lane streams float4 channel
// slices (one 128-byte line per voxel per step), partial dot products are combined with wave shuffles.
#include "act_io.h"
#include "head_bn.h"

namespace {

constexpr int G = 8;   // lanes per voxel

__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// NOUT = 3: plain head.  NOUT = 6: rows 0-2 mu, rows 3-5 sigma pre-activation.
// BN: the head on the PRE-NORM tensor of the ConvUnit in front of it (PULPoEncoder.sample_merge_block -> mu_sigma, VelocityField's last unit -> its
// 1x1x1 convolution).  That unit's output z = lrelu(scale * y + shift) has no reader but the head, and the gradient dz the head sends back none but
// the unit's BatchNorm backward: both are formed where they are used (z: three operations per element in kernels that wait for memory; dz: 3 - 6
// products per element from planar values the kernels hold anyway), so the chain reads y three times and writes dy once instead of ten passes.
// h is then y (fp32), coef the unit's coefficient block (pulpo_bn_fwd_finalize), and the load applies pulpo::bn_lrelu from scale / shift in LDS.
template <int NOUT, bool VEC, bool BN, typename TH = float>
__global__ __launch_bounds__(256) void heads_fwd_kernel(const TH* __restrict__ h, long ps, const float* __restrict__ coef, float slope,
                                                          const float* __restrict__ Wt, const float* __restrict__ bias, const float* __restrict__ eps,
                                                          float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2, int B, long V, int C) {
    extern __shared__ float wl[];              // [NOUT][C] weights | (BN) [C] scale | [C] shift
    float* scl = wl + NOUT * C;
    float* shl = scl + C;
    for (int j = threadIdx.x; j < NOUT * C; j += blockDim.x) wl[j] = Wt[j];
    if constexpr (BN)
        for (int j = threadIdx.x; j < C; j += blockDim.x) { scl[j] = coef[2 * C + j]; shl[j] = coef[3 * C + j]; }
    __syncthreads();
    const int g = threadIdx.x & (G - 1);
    const long npix = (long)B * V;
    const long pstep = (long)gridDim.x * (blockDim.x / G);
    for (long p0 = (long)blockIdx.x * (blockDim.x / G); p0 < npix; p0 += pstep) {   // uniform trip count per block
        const long p = p0 + threadIdx.x / G;
        const bool live = p < npix;
        float acc[NOUT];
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] = 0.f;
        if (live) {
            const TH* hp = h + p * ps;
            constexpr int NV = VEC ? 4 : 1;
            for (int c = NV * g; c < C; c += NV * G) {
                float x[NV];
                pulpo::ldv<NV>(hp + c, x);
                if constexpr (BN) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) x[k] = pulpo::bn_lrelu(x[k], scl[c + k], shl[c + k], slope);
                }
#pragma unroll
                for (int j = 0; j < NOUT; ++j) {
                    const float* w = wl + j * C + c;
                    if constexpr (VEC) acc[j] += x[0] * w[0] + x[1] * w[1] + x[2] * w[2] + x[3] * w[3];
                    else acc[j] += x[0] * w[0];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] = group_sum(acc[j]);
        // every lane of the group holds the sums (xor shuffles): lane g < 3 finishes output component g - one load / store instruction per output
        // tensor and trip instead of three from the group's first lane (the kernel ran at what the vector-memory unit issues, not at what HBM delivers)
        if (live && g < 3) {
            const long b = p / V, v = p - b * V;
            const long at = b * 3 * V + v + g * V;
            const float a_lo = g == 0 ? acc[0] : g == 1 ? acc[1] : acc[2];
            if constexpr (NOUT == 3) {
                o0[at] = a_lo + bias[g];
            } else {
                const float a_hi = g == 0 ? acc[3] : g == 1 ? acc[4] : acc[5];
                const float mu = a_lo + bias[g];
                const float sg = softplus_f(a_hi + bias[3 + g]);
                o0[at] = mu;
                o1[at] = sg;
                o2[at] = eps != nullptr ? mu + sg * eps[at] : mu;
            }
        }
    }
}

// The five planar 3-channel operands of a pixel (upstream gradients of mu / sigma / z, the noise, sigma) are the same 15 values for every
// thread of the pixel's row.  Loaded by each thread they were 15 of the 16 load instructions a wave issued per trip, and the kernels ran at
// what the vector-memory unit issues (2.3 TB/s at 96 channels) instead of what HBM delivers: the row's first threads fetch them once into
// sv16[slot][0..14] (absent operands stored as 0), the row reads them from LDS behind the trip's barrier (two buffers by trip parity: one barrier per trip).
__device__ __forceinline__ void stage_head_operands(float (*sv16)[16], int slot, int col, int CV, const float* g0, const float* g1, const float* g2, const float* eps,
                                                    const float* sigma, long base, long V) {
    for (int q = col; q < 15; q += CV) {
        const int arr = q / 3, j = q - 3 * arr;
        const float* src = arr == 0 ? g0 : arr == 1 ? g1 : arr == 2 ? g2 : arr == 3 ? eps : sigma;
        sv16[slot][q] = src != nullptr ? src[base + j * V] : 0.f;
    }
}

// backward.  dpre[j] (j < NOUT) per voxel is formed from the upstream gradients:
//   NOUT == 3 : dpre = g0
//   NOUT == 6 : dmu = g0 + g2 ; dsigma = g1 + g2 * eps ; dpre[3+j] = dsigma * (1 - exp(-sigma))   (softplus' = sigmoid)
// outputs: dh[pixel][C] ;  partial[blk][NOUT*C + NOUT] = per-block sums for dW and db.
// Thread (col,row) owns VEC channels and walks the block's pixels, so dW accumulates in NOUT*VEC registers.
// BN: the backward of the head AND the first pass of the unit's BatchNorm / LeakyReLU backward (bn_lrelu_bwd_reduce_kernel): h is the pre-norm
// tensor y; the thread forms z for dW and dz = sum_j dpre[j] * W[j][c] for
//   dbn = dz * lrelu'(scale * y + shift);   bnpart[blk][0][c] = sum dbn,  bnpart[blk][1][c] = sum dbn * (y - m32)
// (pulpo::bn_bwd_reduce_step; rows as pulpo_bn_bwd_finalize reads them) and stores no dh.  Fixed block partition, fixed summation order: the
// same bits on every run.  The row count is blockDim.x / CV (the BN launcher may start fewer than 256 threads).
template <int NOUT, int VEC, bool BN, typename TH = float>
__global__ __launch_bounds__(256) void heads_bwd_kernel(const TH* __restrict__ h, long ps, const float* __restrict__ coef, float slope,
                                                          const float* __restrict__ Wt, const float* __restrict__ g0, const float* __restrict__ g1,
                                                          const float* __restrict__ g2, const float* __restrict__ eps, const float* __restrict__ sigma,
                                                          TH* __restrict__ dh, long dps, float* __restrict__ partial, float* __restrict__ bnpart, int B, long V,
                                                          int C) {
    extern __shared__ float red[];             // [RB][NOUT*C + NOUT (+ 2*C)] | (NOUT 6) [2 * RB][16] planar operands (sized by the launcher)
    const int CV = C / VEC, RB = blockDim.x / CV;
    const int col = threadIdx.x % CV, row = threadIdx.x / CV;
    const int c = col * VEC;
    const int ROWLEN = NOUT * C + NOUT, ROWLEN2 = ROWLEN + (BN ? 2 * C : 0);
    const long npix = (long)B * V;
    const bool mine = row < RB;
    float dw[NOUT][VEC], db[NOUT], w[NOUT][VEC], sc[VEC], sh[VEC], m32[VEC], s0[VEC], s1[VEC];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        db[j] = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) { dw[j][k] = 0.f; w[j][k] = mine ? Wt[j * C + c + k] : 0.f; }
    }
    if constexpr (BN) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            s0[k] = s1[k] = 0.f;
            sc[k] = mine ? coef[2 * C + c + k] : 0.f;
            sh[k] = mine ? coef[3 * C + c + k] : 0.f;
            m32[k] = mine ? coef[c + k] : 0.f;
        }
    }
    // one pixel: v = h (BN: y), dpre = the head's pre-activation gradients
    auto pixel = [&](long p, const float (&v)[VEC], const float (&dpre)[NOUT]) {
        float x[VEC], o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) { x[k] = BN ? pulpo::bn_lrelu(v[k], sc[k], sh[k], slope) : v[k]; o[k] = 0.f; }
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            db[j] += dpre[j];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                // (BN: dz spelled fmaf - bn_lrelu_bwd_apply_heads_kernel forms the same bits again; the stored dh keeps the expression it always had,
                //  which the compiler does not contract everywhere)
                if constexpr (BN) o[k] = fmaf(dpre[j], w[j][k], o[k]);
                else o[k] += dpre[j] * w[j][k];
                dw[j][k] = fmaf(dpre[j], x[k], dw[j][k]);
            }
        }
        if constexpr (BN) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) pulpo::bn_bwd_reduce_step(o[k], v[k], sc[k], sh[k], m32[k], slope, s0[k], s1[k]);
        } else {
            pulpo::stv<VEC>(dh + p * dps + c, o);
        }
    };
    if constexpr (NOUT == 6) {
        float (*sv16)[16] = reinterpret_cast<float (*)[16]>(red + (size_t)RB * ROWLEN2);       // [2 * RB][16], behind the reduction rows
        int it = 0;
        for (long pb = (long)blockIdx.x * RB; pb < npix; pb += (long)gridDim.x * RB, it ^= 1) {     // uniform trip count per block for the barrier
            const long p = pb + row;
            const bool live = mine && p < npix;
            const long pc = live ? p : 0;
            const long b = pc / V, v_ = pc - b * V;
            if (live) stage_head_operands(sv16, it * RB + row, col, CV, g0, g1, g2, eps, sigma, b * 3 * V + v_, V);
            float v[VEC];
            if (live) pulpo::ldv<VEC>(h + p * ps + c, v);
            __syncthreads();
            if (live) {
                float dpre[6];
                pulpo::head_dpre6(sv16[it * RB + row], dpre);                  // dmu = g0 + g2 ; dsigma = g1 + g2 * eps (eps absent: stored as 0)
                pixel(p, v, dpre);
            }
        }
    } else if (mine) {
        for (long p = (long)blockIdx.x * RB + row; p < npix; p += (long)gridDim.x * RB) {
            const long b = p / V, v_ = p - b * V;
            const long base = b * 3 * V + v_;
            float dpre[NOUT], v[VEC];
#pragma unroll
            for (int j = 0; j < 3; ++j) dpre[j] = g0[base + j * V];
            pulpo::ldv<VEC>(h + p * ps + c, v);
            pixel(p, v, dpre);
        }
    }
    if (mine) {
        float* r = red + (size_t)row * ROWLEN2;
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[j * C + c + k] = dw[j][k];
            if (col == 0) r[NOUT * C + j] = db[j];
        }
        if constexpr (BN) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) { r[ROWLEN + c + k] = s0[k]; r[ROWLEN + C + c + k] = s1[k]; }
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ROWLEN2; j += blockDim.x) {
        float t = 0.f;
        for (int r = 0; r < RB; ++r) t += red[(size_t)r * ROWLEN2 + j];
        if (!BN || j < ROWLEN) partial[(long)blockIdx.x * ROWLEN + j] = t;
        else bnpart[(long)blockIdx.x * 2 * C + (j - ROWLEN)] = t;
    }
}

// second pass of that BatchNorm backward (bn_lrelu_bwd_apply_kernel) with dz formed per element from the head's planar operands:
//   dy = A * dbn + B * (y - m32) + C  with the constants of pulpo::bn_bwd_constants in LDS;  partial2[blk][c] = sum dy (conv-bias gradient).
// dy: channel c of pixel p at (c / 8) * dykb + p * dyps + c % 8 (dykb = 8: channels-last; else the channel-blocked layout, see pulpo_bn_lrelu_bwd_apply_kb_t)
template <int NOUT, int VEC>
__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_heads_kernel(const float* __restrict__ y, long yps, const float* __restrict__ coef,
                                                                         const double* __restrict__ totd, float slope, const float* __restrict__ Wt,
                                                                         const float* __restrict__ g0, const float* __restrict__ g1, const float* __restrict__ g2,
                                                                         const float* __restrict__ eps, const float* __restrict__ sigma, float* __restrict__ dy,
                                                                         long dyps, long dykb, float* __restrict__ partial2, int B, long V, int C) {
    extern __shared__ float red[];             // [RB][C] sums of dy | [6][C] constants | [NOUT][C] head weights | (NOUT 6) [2 * RB][16] planar operands
    const int CV = C / VEC, RB = blockDim.x / CV;
    const int col = threadIdx.x % CV, row = threadIdx.x / CV;
    const int c = col * VEC;
    const long npix = (long)B * V;
    const bool mine = row < RB;
    float* kst = red + RB * C;
    float* wl = kst + 6 * C;
    float (*sv16)[16] = reinterpret_cast<float (*)[16]>(wl + NOUT * C);
    pulpo::bn_bwd_constants(kst, coef, totd, C);
    for (int j = threadIdx.x; j < NOUT * C; j += blockDim.x) wl[j] = Wt[j];
    __syncthreads();
    float s0[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s0[k] = 0.f;
    const long cdst = (long)(c >> 3) * dykb + (c & 7);
    int it = 0;
    for (long pb = (long)blockIdx.x * RB; pb < npix; pb += (long)gridDim.x * RB, it ^= 1) {     // uniform trip count per block (NOUT 6: one barrier per trip)
        const long p = pb + row;
        const bool live = mine && p < npix;
        const long pc = live ? p : 0;
        const long b = pc / V, v_ = pc - b * V;
        const long base = b * 3 * V + v_;
        float dpre[NOUT], v[VEC], g[VEC], o[VEC];
        if constexpr (NOUT == 6) {
            if (live)                               // (own text of stage_head_operands: the call costs this kernel 4 SGPRs and 0.0025 ms of 0.024 per launch, profiles/epilogue_share_ab.txt)
                for (int q = col; q < 15; q += CV) {
                    const int arr = q / 3, j = q - 3 * arr;
                    const float* src = arr == 0 ? g0 : arr == 1 ? g1 : arr == 2 ? g2 : arr == 3 ? eps : sigma;
                    sv16[it * RB + row][q] = src != nullptr ? src[base + j * V] : 0.f;
                }
            if (live) pulpo::ldv<VEC>(y + p * yps + c, v);
            __syncthreads();
            if (live) pulpo::head_dpre6(sv16[it * RB + row], dpre);
        } else if (live) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dpre[j] = g0[base + j * V];
            pulpo::ldv<VEC>(y + p * yps + c, v);
        }
        if (!live) continue;
        int cl = c;                                 // (opaque: the constants are READ here every time, not kept in registers - see bn_lrelu_bwd_apply_kernel)
        asm volatile("" : "+v"(cl));
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = 0.f;
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {            // dz, the expression of heads_bwd_kernel
            float wj[VEC];
            pulpo::ldv<VEC>(wl + j * C + cl, wj);
#pragma unroll
            for (int k = 0; k < VEC; ++k) g[k] = fmaf(dpre[j], wj[k], g[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            float sh[VEC], sc[VEC];
            pulpo::ldv<VEC>(kst + 0 * C + cl, sc);
            pulpo::ldv<VEC>(kst + 1 * C + cl, sh);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float bn = v[k] * sc[k] + sh[k];
                g[k] = sc[k] * (bn > 0.f ? g[k] : g[k] * slope);          // scale * dbn
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            float m32[VEC], cb[VEC], chi[VEC];
            pulpo::ldv<VEC>(kst + 2 * C + cl, m32);
            pulpo::ldv<VEC>(kst + 3 * C + cl, cb);
            pulpo::ldv<VEC>(kst + 4 * C + cl, chi);
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = fmaf(cb[k], v[k] - m32[k], chi[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            float clo[VEC];
            pulpo::ldv<VEC>(kst + 5 * C + cl, clo);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                o[k] = (g[k] + v[k]) + clo[k];
                s0[k] += o[k];
            }
        }
        pulpo::stv<VEC>(dy + p * dyps + cdst, o);
    }
    if (mine) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) red[row * C + c + k] = s0[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C; j += blockDim.x) {
        float t = 0.f;
        for (int r = 0; r < RB; ++r) t += red[r * C + j];
        partial2[(long)blockIdx.x * C + j] = t;
    }
}

inline int heads_blocks(long npix) { return (int)std::max<long>(1, std::min<long>((npix + 31) / 32, 1024)); }

}  // namespace

// Wt: [NOUT][C] (rows 0-2 = first conv, rows 3-5 = second conv for NOUT == 6); bias: [NOUT].  h_dt: dtype code of h (0 fp32, 1 bf16;
// stride in elements); the outputs are planar fp32
PULPO_API int pulpo_heads_fwd_t(const void* h, int h_dt, int64_t ps, const float* Wt, const float* bias, const float* eps, float* o0, float* o1,
                                float* o2, int nout, int B, int64_t V, int C, void* stream) {
    PULPO_REQUIRE(h && Wt && bias && o0 && B > 0 && V > 0 && C > 0, "heads_fwd: bad arguments");
    PULPO_REQUIRE(nout == 3 || (nout == 6 && o1 && o2), "heads_fwd: nout must be 3 or 6");
    PULPO_REQUIRE_DT(h_dt, "heads_fwd");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && ps % 4 == 0 && (((uintptr_t)h) % (h_dt ? 8 : 16)) == 0;
    const int nblk = heads_blocks((long)B * V);
    const size_t lds = (size_t)nout * C * sizeof(float);
    PULPO_DISPATCH_DT(h_dt, TH, {
        const TH* hp = (const TH*)h;
        if (nout == 3) {
            if (vec) hipLaunchKernelGGL((heads_fwd_kernel<3, true, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, bias, eps, o0, o1, o2, B, V, C);
            else hipLaunchKernelGGL((heads_fwd_kernel<3, false, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, bias, eps, o0, o1, o2, B, V, C);
        } else {
            if (vec) hipLaunchKernelGGL((heads_fwd_kernel<6, true, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, bias, eps, o0, o1, o2, B, V, C);
            else hipLaunchKernelGGL((heads_fwd_kernel<6, false, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, bias, eps, o0, o1, o2, B, V, C);
        }
    });
    return pulpo::check_launch("heads_fwd");
}

PULPO_API int pulpo_heads_fwd(const float* h, int64_t ps, const float* Wt, const float* bias, const float* eps, float* o0, float* o1,
                              float* o2, int nout, int B, int64_t V, int C, void* stream) {
    return pulpo_heads_fwd_t(h, 0, ps, Wt, bias, eps, o0, o1, o2, nout, B, V, C, stream);
}

PULPO_API int pulpo_heads_bwd_blocks(int B, int64_t V, int C) {
    const int vec = (C % 4 == 0) ? 4 : 1;
    const int RB = std::max(1, 256 / (C / vec));
    const long npix = (long)B * V;
    return (int)std::max<long>(1, std::min<long>((npix + RB * 8 - 1) / (RB * 8), 1024));
}

// partial: [pulpo_heads_bwd_blocks][nout*C + nout]; reduce with pulpo_colsum -> (dW[nout][C] | db[nout]).  h and dh share the dtype h_dt.
PULPO_API int pulpo_heads_bwd_t(const void* h, int h_dt, int64_t ps, const float* Wt, const float* g0, const float* g1, const float* g2,
                                const float* eps, const float* sigma, void* dh, int64_t dps, float* partial, int nout, int B, int64_t V, int C,
                                void* stream) {
    PULPO_REQUIRE(h && Wt && dh && partial && B > 0 && V > 0 && C > 0, "heads_bwd: bad arguments");
    PULPO_REQUIRE((nout == 3 && g0) || (nout == 6 && sigma), "heads_bwd: nout must be 3 (with g0) or 6 (with sigma)");
    PULPO_REQUIRE_DT(h_dt, "heads_bwd");
    hipStream_t st = (hipStream_t)stream;
    // unaligned operands (a channel slice of a wider channels-last buffer at an odd offset, which the forward takes with its scalar loads) take the
    // VEC = 1 instance like the forward does, instead of refusing a tensor whose forward pass already ran
    const bool v4 = C % 4 == 0 && ps % 4 == 0 && dps % 4 == 0 && ((((uintptr_t)h) | ((uintptr_t)dh)) % (h_dt ? 8 : 16)) == 0;
    PULPO_REQUIRE(C / (v4 ? 4 : 1) <= 256, "heads_bwd: too many channels (%d%s)", C, v4 || C % 4 != 0 ? "" : ", unaligned operands");
    const int nblk = pulpo_heads_bwd_blocks(B, V, C);
    const int RB = std::max(1, 256 / (C / (v4 ? 4 : 1)));
    const size_t lds = ((size_t)RB * (nout * C + nout) + (nout == 6 ? (size_t)2 * RB * 16 : 0)) * sizeof(float);       // reduction rows + (nout 6) the per-pixel operand rows
    PULPO_REQUIRE(lds <= 64 * 1024, "heads_bwd: LDS budget exceeded");
    PULPO_DISPATCH_DT(h_dt, TH, {
        const TH* hp = (const TH*)h;
        TH* dhp = (TH*)dh;
        if (nout == 3) {
            if (v4) hipLaunchKernelGGL((heads_bwd_kernel<3, 4, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, g0, g1, g2, eps, sigma, dhp, dps, partial, nullptr, B, V, C);
            else hipLaunchKernelGGL((heads_bwd_kernel<3, 1, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, g0, g1, g2, eps, sigma, dhp, dps, partial, nullptr, B, V, C);
        } else {
            if (v4) hipLaunchKernelGGL((heads_bwd_kernel<6, 4, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, g0, g1, g2, eps, sigma, dhp, dps, partial, nullptr, B, V, C);
            else hipLaunchKernelGGL((heads_bwd_kernel<6, 1, false, TH>), dim3(nblk), dim3(256), lds, st, hp, ps, nullptr, 0.f, Wt, g0, g1, g2, eps, sigma, dhp, dps, partial, nullptr, B, V, C);
        }
    });
    return pulpo::check_launch("heads_bwd");
}

PULPO_API int pulpo_heads_bwd(const float* h, int64_t ps, const float* Wt, const float* g0, const float* g1, const float* g2, const float* eps,
                              const float* sigma, float* dh, int64_t dps, float* partial, int nout, int B, int64_t V, int C, void* stream) {
    return pulpo_heads_bwd_t(h, 0, ps, Wt, g0, g1, g2, eps, sigma, dh, dps, partial, nout, B, V, C, stream);
}

// ---- the same heads on the pre-norm tensor y of the ConvUnit in front of them (fp32, strides in elements; coef: that unit's coefficient block,
// slope: its LeakyReLU).  Channel groups of four where C % 4 == 0 and everything is 16-byte aligned, else single channels (C <= 256).
PULPO_API int pulpo_heads_fwd_bn_t(const float* y, int64_t ps, const float* coef, float slope, const float* Wt, const float* bias, const float* eps,
                                   float* o0, float* o1, float* o2, int nout, int B, int64_t V, int C, void* stream) {
    PULPO_REQUIRE(y && coef && Wt && bias && o0 && B > 0 && V > 0 && C > 0, "heads_fwd_bn: bad arguments");
    PULPO_REQUIRE(nout == 3 || (nout == 6 && o1 && o2), "heads_fwd_bn: nout must be 3 or 6");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && ps % 4 == 0 && (((uintptr_t)y) % 16) == 0;
    const int nblk = heads_blocks((long)B * V);
    const size_t lds = (size_t)(nout + 2) * C * sizeof(float);
    PULPO_REQUIRE(lds <= 64 * 1024, "heads_fwd_bn: LDS budget exceeded");
    if (nout == 3) {
        if (vec) hipLaunchKernelGGL((heads_fwd_kernel<3, true, true>), dim3(nblk), dim3(256), lds, st, y, ps, coef, slope, Wt, bias, eps, o0, o1, o2, B, V, C);
        else hipLaunchKernelGGL((heads_fwd_kernel<3, false, true>), dim3(nblk), dim3(256), lds, st, y, ps, coef, slope, Wt, bias, eps, o0, o1, o2, B, V, C);
    } else {
        if (vec) hipLaunchKernelGGL((heads_fwd_kernel<6, true, true>), dim3(nblk), dim3(256), lds, st, y, ps, coef, slope, Wt, bias, eps, o0, o1, o2, B, V, C);
        else hipLaunchKernelGGL((heads_fwd_kernel<6, false, true>), dim3(nblk), dim3(256), lds, st, y, ps, coef, slope, Wt, bias, eps, o0, o1, o2, B, V, C);
    }
    return pulpo::check_launch("heads_fwd_bn");
}

// partial: [pulpo_heads_bwd_blocks][nout*C + nout] as pulpo_heads_bwd_t; bnpart: [pulpo_heads_bwd_blocks][2][C], the rows pulpo_bn_bwd_finalize takes
// (nrow = pulpo_heads_bwd_blocks).  The gradient of the unit's output is not written: pulpo_bn_lrelu_bwd_apply_heads_t forms it again.
PULPO_API int pulpo_heads_bwd_bn_t(const float* y, int64_t ps, const float* coef, float slope, const float* Wt, const float* g0, const float* g1,
                                   const float* g2, const float* eps, const float* sigma, float* partial, float* bnpart, int nout, int B, int64_t V, int C,
                                   void* stream) {
    PULPO_REQUIRE(y && coef && Wt && partial && bnpart && B > 0 && V > 0 && C > 0, "heads_bwd_bn: bad arguments");
    PULPO_REQUIRE((nout == 3 && g0) || (nout == 6 && sigma), "heads_bwd_bn: nout must be 3 (with g0) or 6 (with sigma)");
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = C % 4 == 0 && ps % 4 == 0 && (((uintptr_t)y) % 16) == 0;
    PULPO_REQUIRE(C / (v4 ? 4 : 1) <= 256, "heads_bwd_bn: too many channels (%d%s)", C, v4 || C % 4 != 0 ? "" : ", unaligned operands");
    const int nblk = pulpo_heads_bwd_blocks(B, V, C);
    const int CV = C / (v4 ? 4 : 1);
    int RB = std::max(1, 256 / CV);
    auto lds_of = [&](int rb) { return ((size_t)rb * (nout * C + nout + 2 * C) + (nout == 6 ? (size_t)2 * rb * 16 : 0)) * sizeof(float); };
    // (a handful of channels: 256 pixel rows of sums and planar operands pass 64 KB - fewer rows per workgroup, i.e. fewer threads; the kernel takes its
    //  row count from the launch and walks the pixels in grid strides)
    while (RB > 1 && lds_of(RB) > 64 * 1024) RB /= 2;
    const size_t lds = lds_of(RB);
    PULPO_REQUIRE(lds <= 64 * 1024, "heads_bwd_bn: LDS budget exceeded");
    const int nthr = RB == std::max(1, 256 / CV) ? 256 : RB * CV;          // (the kernel's row count is blockDim.x / CV)
    if (nout == 3) {
        if (v4) hipLaunchKernelGGL((heads_bwd_kernel<3, 4, true>), dim3(nblk), dim3(nthr), lds, st, y, ps, coef, slope, Wt, g0, g1, g2, eps, sigma, (float*)nullptr, 0L, partial, bnpart, B, V, C);
        else hipLaunchKernelGGL((heads_bwd_kernel<3, 1, true>), dim3(nblk), dim3(nthr), lds, st, y, ps, coef, slope, Wt, g0, g1, g2, eps, sigma, (float*)nullptr, 0L, partial, bnpart, B, V, C);
    } else {
        if (v4) hipLaunchKernelGGL((heads_bwd_kernel<6, 4, true>), dim3(nblk), dim3(nthr), lds, st, y, ps, coef, slope, Wt, g0, g1, g2, eps, sigma, (float*)nullptr, 0L, partial, bnpart, B, V, C);
        else hipLaunchKernelGGL((heads_bwd_kernel<6, 1, true>), dim3(nblk), dim3(nthr), lds, st, y, ps, coef, slope, Wt, g0, g1, g2, eps, sigma, (float*)nullptr, 0L, partial, bnpart, B, V, C);
    }
    return pulpo::check_launch("heads_bwd_bn");
}

PULPO_API int pulpo_bn_bwd_blocks(int64_t npix, int C);      // (norm_act.hip)

namespace {
int apply_heads(const float* y, long yps, const float* coef, const double* totd, float slope, const float* Wt, const float* g0, const float* g1, const float* g2,
                const float* eps, const float* sigma, float* dy, long dyps, long dykb, float* partial2, int nout, int B, long V, int C, hipStream_t st) {
    const bool v4 = C % 4 == 0 && yps % 4 == 0 && dyps % 4 == 0 && dykb % 4 == 0 && ((((uintptr_t)y) | ((uintptr_t)dy)) % 16) == 0;
    if (C / (v4 ? 4 : 1) > 256) return pulpo::fail(-1, "bn_lrelu_bwd_apply_heads: too many channels (%d%s)", C, v4 || C % 4 != 0 ? "" : ", unaligned operands");
    const int nblk = pulpo_bn_bwd_blocks((long)B * V, C);
    const int RB = std::max(1, 256 / (C / (v4 ? 4 : 1)));
    const size_t lds = ((size_t)(RB + 6 + nout) * C + (nout == 6 ? (size_t)2 * RB * 16 : 0)) * sizeof(float);
    if (lds > 64 * 1024) return pulpo::fail(-1, "bn_lrelu_bwd_apply_heads: LDS budget exceeded");
    if (nout == 3) {
        if (v4) hipLaunchKernelGGL((bn_lrelu_bwd_apply_heads_kernel<3, 4>), dim3(nblk), dim3(256), lds, st, y, yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, dyps, dykb, partial2, B, V, C);
        else hipLaunchKernelGGL((bn_lrelu_bwd_apply_heads_kernel<3, 1>), dim3(nblk), dim3(256), lds, st, y, yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, dyps, dykb, partial2, B, V, C);
    } else {
        if (v4) hipLaunchKernelGGL((bn_lrelu_bwd_apply_heads_kernel<6, 4>), dim3(nblk), dim3(256), lds, st, y, yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, dyps, dykb, partial2, B, V, C);
        else hipLaunchKernelGGL((bn_lrelu_bwd_apply_heads_kernel<6, 1>), dim3(nblk), dim3(256), lds, st, y, yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, dyps, dykb, partial2, B, V, C);
    }
    return pulpo::check_launch("bn_lrelu_bwd_apply_heads");
}
}  // namespace

// the second BatchNorm-backward pass of that unit: totd from pulpo_bn_bwd_finalize over bnpart; partial2: [pulpo_bn_bwd_blocks(B * V, C)][C] as
// pulpo_bn_lrelu_bwd_apply_t.  The head's operands as pulpo_heads_bwd_bn_t took them.
PULPO_API int pulpo_bn_lrelu_bwd_apply_heads_t(const float* y, int64_t yps, const float* coef, const double* totd, float slope, const float* Wt, const float* g0,
                                               const float* g1, const float* g2, const float* eps, const float* sigma, float* dy, int64_t dyps, float* partial2,
                                               int nout, int B, int64_t V, int C, void* stream) {
    PULPO_REQUIRE(y && coef && totd && Wt && dy && partial2 && B > 0 && V > 0 && C > 0, "bn_lrelu_bwd_apply_heads: bad arguments");
    PULPO_REQUIRE((nout == 3 && g0) || (nout == 6 && sigma), "bn_lrelu_bwd_apply_heads: nout must be 3 (with g0) or 6 (with sigma)");
    return apply_heads(y, (long)yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, (long)dyps, 8, partial2, nout, B, (long)V, C, (hipStream_t)stream);
}

// ... with dy in the channel-blocked layout [C / 8][pixels][8] (dyps = 8, dykb = pixels * 8; C % 8 == 0), as pulpo_bn_lrelu_bwd_apply_kb_t
PULPO_API int pulpo_bn_lrelu_bwd_apply_heads_kb_t(const float* y, int64_t yps, const float* coef, const double* totd, float slope, const float* Wt,
                                                  const float* g0, const float* g1, const float* g2, const float* eps, const float* sigma, float* dy,
                                                  int64_t dyps, int64_t dykb, float* partial2, int nout, int B, int64_t V, int C, void* stream) {
    PULPO_REQUIRE(y && coef && totd && Wt && dy && partial2 && B > 0 && V > 0 && C > 0, "bn_lrelu_bwd_apply_heads_kb: bad arguments");
    PULPO_REQUIRE((nout == 3 && g0) || (nout == 6 && sigma), "bn_lrelu_bwd_apply_heads_kb: nout must be 3 (with g0) or 6 (with sigma)");
    PULPO_REQUIRE(C % 8 == 0 && dyps % 4 == 0 && dyps >= 8 && dykb % 4 == 0 && dykb >= 8, "bn_lrelu_bwd_apply_heads_kb: C %% 8 == 0, strides in whole four-channel groups");
    return apply_heads(y, (long)yps, coef, totd, slope, Wt, g0, g1, g2, eps, sigma, dy, (long)dyps, (long)dykb, partial2, nout, B, (long)V, C, (hipStream_t)stream);
}
