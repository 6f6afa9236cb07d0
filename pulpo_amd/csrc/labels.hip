// Warping an integer label map as if it were one-hot, for the Monte-Carlo evaluation of segmentations (evaluate.py:252-274, 2-D branch;
// the 3-D branch gives them up for memory, evaluate.py:208).  The operation is warp3d(df, one_hot(labels, C)): per output voxel the
// probability of class c is the sum of the trilinear corner weights whose corner carries label c.  The coordinate (sampling.h) and the
// weight products are warp.hip's, in the same order; a one-hot channel multiplies every weight by 0 or 1 exactly, so the per-class sum
// of the matching weights, added in corner order, is bitwise what warp_fwd_kernel computes on the one-hot map.
// One thread per output voxel: displacement planes coalesced, 8 one- or four-byte corner gathers from L1/L2, the <= 8 distinct classes
// deduplicated in registers.  Optional outputs, each selected by a nullable pointer: the dense one-hot warp, the arg-max label, per-class
// Dice sums against a target label map and a Welford update of per-(class, voxel) moments (the arithmetic of pulpo_mc_moments_update).
// Dice sums are 64-bit fixed point (weights in units of 2^-32, target counts as integers): integer adds are associative, so the wave
// reduction, the LDS adds and the one global add per block and class give the same bits in any order.
#include "common.h"
#include "sampling.h"

namespace {

using pulpo::Corner;
using pulpo::sample_coord;

constexpr int kMaxClasses = 256;
constexpr double kFix = 4294967296.0;        // 2^32: fixed-point unit of the Dice weight sums

using pulpo::eblocks;

__device__ __forceinline__ unsigned long long to_fix(float p) { return (unsigned long long)__float2ull_rn(p * 4294967296.f); }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename LT>
__device__ __forceinline__ int load_label(const LT* p, long i) { return (int)p[i]; }

// grid (nblk, B); sums: (B, C, 3) u64 = (sum p t, sum t^2, sum p^2) for p = warped one-hot, t = one-hot of the target
template <typename LT>
__global__ __launch_bounds__(256) void warp_labels_kernel(const float* __restrict__ df, const LT* __restrict__ lab, int C, const LT* __restrict__ tgt,
                                                            float* __restrict__ onehot, LT* __restrict__ amax, float* __restrict__ mean,
                                                            float* __restrict__ m2, int k, unsigned long long* __restrict__ sums, int* __restrict__ flag,
                                                            int Dg, int Hg, int Wg, int Di, int Hi, int Wi) {
    __shared__ unsigned long long sh[3 * kMaxClasses];
    const int b = blockIdx.y;
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi;
    const LT* lb = lab + b * Vi;
    if (tgt != nullptr) {
        for (int j = threadIdx.x; j < 3 * C; j += 256) sh[j] = 0ull;
        __syncthreads();
    }
    const float inv = 1.f / (float)k;
    bool bad = false;
    // block-uniform trip count: every lane of a wave takes part in the Dice exchange below
    for (long base = (long)blockIdx.x * 256; base < Vg; base += (long)gridDim.x * 256) {
        const long v = base + threadIdx.x;
        const bool valid = v < Vg;
        int cl[8];
        float p[8];
        bool first[8];
        int tc = -1;
        if (valid) {
            const int vi = (int)v;
            const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
            const float* d = df + (long)b * 3 * Vg + v;
            const Corner cz = sample_coord((float)z, d[0], Dg, Di);
            const Corner cy = sample_coord((float)y, d[Vg], Hg, Hi);
            const Corner cx = sample_coord((float)x, d[2 * Vg], Wg, Wi);
            const long o00 = ((long)cz.i0 * Hi + cy.i0) * Wi, o01 = ((long)cz.i0 * Hi + cy.i1) * Wi;
            const long o10 = ((long)cz.i1 * Hi + cy.i0) * Wi, o11 = ((long)cz.i1 * Hi + cy.i1) * Wi;
            const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
            // corner order and weight products of warp_fwd_kernel
            const float w[8] = {wz0 * wy0 * wx0, wz0 * wy0 * cx.f, wz0 * cy.f * wx0, wz0 * cy.f * cx.f,
                                cz.f * wy0 * wx0, cz.f * wy0 * cx.f, cz.f * cy.f * wx0, cz.f * cy.f * cx.f};
            cl[0] = load_label(lb, o00 + cx.i0); cl[1] = load_label(lb, o00 + cx.i1);
            cl[2] = load_label(lb, o01 + cx.i0); cl[3] = load_label(lb, o01 + cx.i1);
            cl[4] = load_label(lb, o10 + cx.i0); cl[5] = load_label(lb, o10 + cx.i1);
            cl[6] = load_label(lb, o11 + cx.i0); cl[7] = load_label(lb, o11 + cx.i1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool ok = cl[i] >= 0 && cl[i] < C;
                bad |= !ok;
                bool f = ok;
#pragma unroll
                for (int h = 0; h < i; ++h) f &= cl[h] != cl[i];
                first[i] = f;
                float s = 0.f;                                 // matching weights added in corner order, starting from 0 like the warp's sum
#pragma unroll
                for (int j = i; j < 8; ++j) s += cl[j] == cl[i] ? w[j] : 0.f;
                p[i] = s;
            }
            if (tgt != nullptr) {
                tc = load_label(tgt, (long)b * Vg + v);
                if (tc < 0 || tc >= C) { bad = true; tc = -1; }
            }
            if (amax != nullptr) {                             // highest probability; ties -> the lowest class
                int bc = C;
                float bp = -1.f;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (first[i] && (p[i] > bp || (p[i] == bp && cl[i] < bc))) { bp = p[i]; bc = cl[i]; }
                amax[(long)b * Vg + v] = (LT)(bc < C ? bc : 0);
            }
            if (onehot != nullptr || mean != nullptr) {
                for (int c = 0; c < C; ++c) {
                    float val = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) val = (first[i] && cl[i] == c) ? p[i] : val;
                    const long oi = ((long)b * C + c) * Vg + v;
                    if (onehot != nullptr) onehot[oi] = val;
                    if (mean != nullptr) {
                        float mu = 0.f, q = 0.f;
                        if (k > 1) { mu = mean[oi]; q = m2[oi]; }
                        pulpo::welford_step(val, mu, q, k, inv);
                        mean[oi] = mu;
                        m2[oi] = q;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) { cl[i] = -1; p[i] = 0.f; first[i] = false; }
        }
        if (tgt != nullptr) {
            // Per class present in the wave: every lane's contribution, one integer wave sum, one LDS add.  The loop runs once per
            // distinct class among the wave's corners and targets (one to three in the interior of a structure).
            unsigned pending = (tc >= 0 ? 0x100u : 0u);
#pragma unroll
            for (int i = 0; i < 8; ++i) pending |= first[i] ? (1u << i) : 0u;
            while (true) {
                const unsigned long long act = __ballot(pending != 0u);
                if (act == 0ull) break;
                int cand = -1;
#pragma unroll
                for (int i = 7; i >= 0; --i) cand = (pending >> i) & 1u ? cl[i] : cand;
                if (cand < 0 && (pending & 0x100u)) cand = tc;
                const int c = __shfl(cand, __ffsll((long long)act) - 1, 64);
                unsigned long long u0 = 0ull, u1 = 0ull, u2 = 0ull;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (((pending >> i) & 1u) && cl[i] == c) {
                        u2 += to_fix(p[i] * p[i]);
                        if (tc == c) u0 += to_fix(p[i]);
                        pending &= ~(1u << i);
                    }
                if ((pending & 0x100u) && tc == c) {
                    u1 = 1ull;
                    pending &= ~0x100u;
                }
                u0 = wave_sum_u64(u0);
                u1 = wave_sum_u64(u1);
                u2 = wave_sum_u64(u2);
                if ((threadIdx.x & 63) == 0) {
                    if (u0) atomicAdd(&sh[3 * c], u0);
                    if (u1) atomicAdd(&sh[3 * c + 1], u1);
                    if (u2) atomicAdd(&sh[3 * c + 2], u2);
                }
            }
        }
    }
    if (bad) atomicOr(flag, 1);
    if (tgt != nullptr) {
        __syncthreads();
        unsigned long long* dst = sums + (long)b * C * 3;
        for (int j = threadIdx.x; j < 3 * C; j += 256)
            if (sh[j]) atomicAdd(dst + j, sh[j]);
    }
}

// dice[b][c] = (2 mean(p t) + 1e-6) / (mean(t^2) + mean(p^2) + 1e-6) over the grid's V voxels: pulpo_dsc's formula for the plane (b, c)
__global__ void dice_from_sums_kernel(const unsigned long long* __restrict__ sums, int n, double V, float* __restrict__ dice) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s0 = (double)sums[3 * i] / kFix, s1 = (double)sums[3 * i + 1], s2 = (double)sums[3 * i + 2] / kFix;
    dice[i] = (float)((2.0 * s0 / V + 1e-6) / (s1 / V + s2 / V + 1e-6));
}

// The level Dice of Evaluate.performance (evaluate.py:1427, 1454-1455) without a one-hot tensor: Soft_dice_loss (src/losses.py:137-145) of
// spatial_transform(df, one_hot(labels)) against F.interpolate(one_hot(target), size = grid, trilinear, align_corners=False).
// Per voxel of the grid, p_c = the sum of the <= 8 corner weights of the warped moving map that carry class c (the coordinates, weight
// products and corner order of warp_labels_kernel) and t_c = the sum of the <= 8 tap weights of the resize that carry class c, with
// PyTorch's source index for size= (resample.hip's src_index: scale = map / grid, src = scale (dst + 0.5) - 0.5 clamped at 0).  Only the
// <= 16 classes met at the voxel have a non-zero p t, p^2 or t^2.  Each per-voxel product is rounded to 64-bit fixed point (units of
// 2^-32) before the integer adds of the wave, the block (LDS) and the grid (one global add per block and class): the same bits in any order.
__device__ __forceinline__ void resize_src_index(int dst, float scale, int in_size, int& i0, int& i1, float& lam) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    lam = s - (float)i0;
}

// grid (nblk, B); sums: (B, C, 3) u64 = (sum p t, sum t^2, sum p^2); labels on (Di, Hi, Wi), target on (Dt, Ht, Wt)
template <typename LT>
__global__ __launch_bounds__(256) void warp_labels_soft_dice_kernel(const float* __restrict__ df, const LT* __restrict__ lab, const LT* __restrict__ tgt,
                                                                      int C, unsigned long long* __restrict__ sums, int* __restrict__ flag, int Dg, int Hg,
                                                                      int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt) {
    __shared__ unsigned long long sh[3 * kMaxClasses];
    const int b = blockIdx.y;
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi, Vt = (long)Dt * Ht * Wt;
    const LT* lb = lab + b * Vi;
    const LT* tb = tgt + b * Vt;
    const float sd = (float)Dt / (float)Dg, shh = (float)Ht / (float)Hg, sw = (float)Wt / (float)Wg;
    for (int j = threadIdx.x; j < 3 * C; j += 256) sh[j] = 0ull;
    __syncthreads();
    bool bad = false;
    // block-uniform trip count: every lane of a wave takes part in the exchange below
    for (long base = (long)blockIdx.x * 256; base < Vg; base += (long)gridDim.x * 256) {
        const long v = base + threadIdx.x;
        int cl[16];          // 0..7 the warp's corners, 8..15 the resize's taps
        float w[16];
        unsigned pending = 0u;
        if (v < Vg) {
            const int vi = (int)v;
            const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
            const float* d = df + (long)b * 3 * Vg + v;
            const Corner cz = sample_coord((float)z, d[0], Dg, Di);
            const Corner cy = sample_coord((float)y, d[Vg], Hg, Hi);
            const Corner cx = sample_coord((float)x, d[2 * Vg], Wg, Wi);
            const long o00 = ((long)cz.i0 * Hi + cy.i0) * Wi, o01 = ((long)cz.i0 * Hi + cy.i1) * Wi;
            const long o10 = ((long)cz.i1 * Hi + cy.i0) * Wi, o11 = ((long)cz.i1 * Hi + cy.i1) * Wi;
            const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
            // corner order and weight products of warp_fwd_kernel
            w[0] = wz0 * wy0 * wx0; w[1] = wz0 * wy0 * cx.f; w[2] = wz0 * cy.f * wx0; w[3] = wz0 * cy.f * cx.f;
            w[4] = cz.f * wy0 * wx0; w[5] = cz.f * wy0 * cx.f; w[6] = cz.f * cy.f * wx0; w[7] = cz.f * cy.f * cx.f;
            cl[0] = load_label(lb, o00 + cx.i0); cl[1] = load_label(lb, o00 + cx.i1);
            cl[2] = load_label(lb, o01 + cx.i0); cl[3] = load_label(lb, o01 + cx.i1);
            cl[4] = load_label(lb, o10 + cx.i0); cl[5] = load_label(lb, o10 + cx.i1);
            cl[6] = load_label(lb, o11 + cx.i0); cl[7] = load_label(lb, o11 + cx.i1);
            int z0, z1, y0, y1, x0, x1;
            float lz, ly, lx;
            resize_src_index(z, sd, Dt, z0, z1, lz);
            resize_src_index(y, shh, Ht, y0, y1, ly);
            resize_src_index(x, sw, Wt, x0, x1, lx);
            const long t00 = ((long)z0 * Ht + y0) * Wt, t01 = ((long)z0 * Ht + y1) * Wt;
            const long t10 = ((long)z1 * Ht + y0) * Wt, t11 = ((long)z1 * Ht + y1) * Wt;
            const float uz0 = 1.f - lz, uy0 = 1.f - ly, ux0 = 1.f - lx;
            w[8] = uz0 * uy0 * ux0; w[9] = uz0 * uy0 * lx; w[10] = uz0 * ly * ux0; w[11] = uz0 * ly * lx;
            w[12] = lz * uy0 * ux0; w[13] = lz * uy0 * lx; w[14] = lz * ly * ux0; w[15] = lz * ly * lx;
            cl[8] = load_label(tb, t00 + x0); cl[9] = load_label(tb, t00 + x1);
            cl[10] = load_label(tb, t01 + x0); cl[11] = load_label(tb, t01 + x1);
            cl[12] = load_label(tb, t10 + x0); cl[13] = load_label(tb, t10 + x1);
            cl[14] = load_label(tb, t11 + x0); cl[15] = load_label(tb, t11 + x1);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool ok = cl[i] >= 0 && cl[i] < C;
                bad |= !ok;
                if (!ok) cl[i] = -1;
                pending |= (ok && w[i] != 0.f) ? (1u << i) : 0u;        // a zero weight adds nothing to any sum
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) { cl[i] = -1; w[i] = 0.f; }
        }
        // Per class present in the wave: every lane's p_c and t_c (matching weights added in corner / tap order, starting from 0 like the
        // warp's sum), three integer wave sums, one LDS add each.  A class is handled once: all its pending bits clear together.
        while (true) {
            const unsigned long long act = __ballot(pending != 0u);
            if (act == 0ull) break;
            int cand = -1;
#pragma unroll
            for (int i = 15; i >= 0; --i) cand = (pending >> i) & 1u ? cl[i] : cand;
            const int c = __shfl(cand, __ffsll((long long)act) - 1, 64);
            float pc = 0.f, tc = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pc += cl[i] == c ? w[i] : 0.f;
                tc += cl[8 + i] == c ? w[8 + i] : 0.f;
                pending &= ~((cl[i] == c ? (1u << i) : 0u) | (cl[8 + i] == c ? (1u << (8 + i)) : 0u));
            }
            const unsigned long long u0 = wave_sum_u64(to_fix(pc * tc)), u1 = wave_sum_u64(to_fix(tc * tc)), u2 = wave_sum_u64(to_fix(pc * pc));
            if ((threadIdx.x & 63) == 0) {
                if (u0) atomicAdd(&sh[3 * c], u0);
                if (u1) atomicAdd(&sh[3 * c + 1], u1);
                if (u2) atomicAdd(&sh[3 * c + 2], u2);
            }
        }
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    unsigned long long* dst = sums + (long)b * C * 3;
    for (int j = threadIdx.x; j < 3 * C; j += 256)
        if (sh[j]) atomicAdd(dst + j, sh[j]);
}

// one wave: dice[b][c] = (2 sum(p t) + 1e-6) / (sum(t^2) + sum(p^2) + 1e-6) (sums, not pulpo_dsc's means) and their mean over (b, c),
// lane t taking planes t, t + 64, ... in that order, then the butterfly
__global__ void soft_dice_from_sums_kernel(const unsigned long long* __restrict__ sums, int n, float* __restrict__ dice, float* __restrict__ mean) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const double s0 = (double)sums[3 * i] / kFix, s1 = (double)sums[3 * i + 1] / kFix, s2 = (double)sums[3 * i + 2] / kFix;
        const double d = (2.0 * s0 + 1e-6) / (s1 + s2 + 1e-6);
        dice[i] = (float)d;
        acc += d;
    }
    acc = pulpo::wave_sum_d(acc);
    if (threadIdx.x == 0) mean[0] = (float)(acc / n);
}

template <typename LT>
__global__ __launch_bounds__(256) void labels_check_kernel(const LT* __restrict__ lab, long n, int C, int* __restrict__ flag) {
    bool bad = false;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int l = (int)lab[e];
        bad |= l < 0 || l >= C;
    }
    if (bad) atomicOr(flag, 1);
}

// (B, C, V) fp32 -> (B, V) labels: arg-max over the channels, the lowest class on ties
template <typename LT>
__global__ __launch_bounds__(256) void labels_from_onehot_kernel(const float* __restrict__ seg, LT* __restrict__ out, int C, long V, long total) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long b = e / V, v = e - b * V;
        const float* s = seg + b * C * V + v;
        float best = s[0];
        int bc = 0;
        for (int c = 1; c < C; ++c) {
            const float x = s[(long)c * V];
            if (x > best) { best = x; bc = c; }
        }
        out[e] = (LT)bc;
    }
}

// Evaluate.ncc (evaluate.py:334-353), zero-normed: sum((a - ma) (b - mb)) / ((std(a) n + 1e-15) (std(b) + 1e-15)), population std.
// Pass 1: block partials of (sum a, sum b); pass 2: every block re-sums pass 1 in the same order for the means, then partials of the
// centred (sum da db, sum da^2, sum db^2); the finalize sums those in block order.  All in double, no atomics.
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = pulpo::wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void ncc_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, double* __restrict__ part) {
    __shared__ double sh[4];
    double sa = 0.0, sb = 0.0;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        sa += a[e];
        sb += b[e];
    }
    const double ta = block_sum_d(sa, sh), tb = block_sum_d(sb, sh);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = ta; part[2 * blockIdx.x + 1] = tb; }
}

__global__ __launch_bounds__(256) void ncc_centred_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, const double* __restrict__ part,
                                                            double* __restrict__ part2) {
    __shared__ double sh[4];
    __shared__ double mab[2];
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int k = 0; k < (int)gridDim.x; ++k) { sa += part[2 * k]; sb += part[2 * k + 1]; }
        mab[0] = sa / (double)n;
        mab[1] = sb / (double)n;
    }
    __syncthreads();
    const double ma = mab[0], mb = mab[1];
    double sab = 0.0, saa = 0.0, sbb = 0.0;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const double da = (double)a[e] - ma, db = (double)b[e] - mb;
        sab += da * db;
        saa += da * da;
        sbb += db * db;
    }
    const double t0 = block_sum_d(sab, sh), t1 = block_sum_d(saa, sh), t2 = block_sum_d(sbb, sh);
    if (threadIdx.x == 0) { part2[3 * blockIdx.x] = t0; part2[3 * blockIdx.x + 1] = t1; part2[3 * blockIdx.x + 2] = t2; }
}

__global__ void ncc_finalize_kernel(const double* __restrict__ part2, int nblk, long n, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double sab = 0.0, saa = 0.0, sbb = 0.0;
    for (int k = 0; k < nblk; ++k) { sab += part2[3 * k]; saa += part2[3 * k + 1]; sbb += part2[3 * k + 2]; }
    const double sa = sqrt(saa / (double)n), sb = sqrt(sbb / (double)n);
    out[0] = sab / ((sa * (double)n + 1e-15) * (sb + 1e-15));
}

// ------------------------------------------------------------------------------------------------ Dice term of the training step from label maps
// Soft_dice_loss (src/losses.py:137-145) of warp3d(df, one_hot(labels)) against the resized one-hot target, with its gradient with respect
// to the field.  The forward sums are warp_labels_soft_dice_kernel's; this finisher turns them into the loss
// mean_(b,c)(1 - dice_bc) * scale (scale = Vg / dice_factor), the per-class Dice (the expression of soft_dice_from_sums_kernel) and, per
// (b, c), the two coefficients of dL/dp_c(v) = a t_c(v) + b p_c(v): a = -2 S / den, b = 2 S num / den^2, S = scale / n.  One wave, in double.
__global__ void label_dice_finish_kernel(const unsigned long long* __restrict__ sums, int n, double scale, float* __restrict__ dice,
                                         float* __restrict__ coef, float* __restrict__ loss) {
    double acc = 0.0;
    const double S = scale / n;
    for (int i = threadIdx.x; i < n; i += 64) {
        const double s0 = (double)sums[3 * i] / kFix, s1 = (double)sums[3 * i + 1] / kFix, s2 = (double)sums[3 * i + 2] / kFix;
        const double num = 2.0 * s0 + 1e-6, den = s1 + s2 + 1e-6;
        const double d = num / den;
        dice[i] = (float)d;
        coef[2 * i] = (float)(-2.0 * S / den);
        coef[2 * i + 1] = (float)(2.0 * S * num / (den * den));
        acc += 1.0 - d;
    }
    acc = pulpo::wave_sum_d(acc);
    if (threadIdx.x == 0) loss[0] = (float)(acc / n * scale);
}

// grid (ceil(Vg / 256), B), one thread per grid voxel, x fastest: the three displacement planes read and the three gradient planes written
// coalesced.  The coordinate, the 8 corner labels and weights and the 8 resize taps are warp_labels_soft_dice_kernel's expressions in its
// order, so p_c and t_c are the forward's to the bit.  For corner i of class c_i, G_i = a[c_i] t_{c_i} + b[c_i] p_{c_i} is dL/dw_i; the
// weights are products of (1 - f) and f per axis, so d w_i / d coord_z = -/+ wy wx for the low / high corner, likewise y and x.
// A label outside [0, C) counts for no class and never indexes the table.  No atomics, no reduction: each voxel's gradient is its own.
template <typename LT>
__global__ __launch_bounds__(256) void label_dice_bwd_kernel(const float* __restrict__ df, const LT* __restrict__ lab, const LT* __restrict__ tgt,
                                                               int C, const float* __restrict__ coef, const float* __restrict__ gup,
                                                               float* __restrict__ ddf, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht,
                                                               int Wt) {
    __shared__ float tab[2 * kMaxClasses];          // (a, b) per class of this block's batch element
    const int b = blockIdx.y;
    for (int j = threadIdx.x; j < 2 * C; j += 256) tab[j] = coef[(long)b * 2 * C + j];
    __syncthreads();
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi, Vt = (long)Dt * Ht * Wt;
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= Vg) return;
    const LT* lb = lab + b * Vi;
    const LT* tb = tgt + b * Vt;
    const float sd = (float)Dt / (float)Dg, shh = (float)Ht / (float)Hg, sw = (float)Wt / (float)Wg;
    const int vi = (int)v;
    const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
    const float* d = df + (long)b * 3 * Vg + v;
    const Corner cz = sample_coord((float)z, d[0], Dg, Di);
    const Corner cy = sample_coord((float)y, d[Vg], Hg, Hi);
    const Corner cx = sample_coord((float)x, d[2 * Vg], Wg, Wi);
    const long o00 = ((long)cz.i0 * Hi + cy.i0) * Wi, o01 = ((long)cz.i0 * Hi + cy.i1) * Wi;
    const long o10 = ((long)cz.i1 * Hi + cy.i0) * Wi, o11 = ((long)cz.i1 * Hi + cy.i1) * Wi;
    const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
    int cl[8], tl[8];
    float w[8], u[8];
    w[0] = wz0 * wy0 * wx0; w[1] = wz0 * wy0 * cx.f; w[2] = wz0 * cy.f * wx0; w[3] = wz0 * cy.f * cx.f;
    w[4] = cz.f * wy0 * wx0; w[5] = cz.f * wy0 * cx.f; w[6] = cz.f * cy.f * wx0; w[7] = cz.f * cy.f * cx.f;
    cl[0] = load_label(lb, o00 + cx.i0); cl[1] = load_label(lb, o00 + cx.i1);
    cl[2] = load_label(lb, o01 + cx.i0); cl[3] = load_label(lb, o01 + cx.i1);
    cl[4] = load_label(lb, o10 + cx.i0); cl[5] = load_label(lb, o10 + cx.i1);
    cl[6] = load_label(lb, o11 + cx.i0); cl[7] = load_label(lb, o11 + cx.i1);
    int z0, z1, y0, y1, x0, x1;
    float lz, ly, lx;
    resize_src_index(z, sd, Dt, z0, z1, lz);
    resize_src_index(y, shh, Ht, y0, y1, ly);
    resize_src_index(x, sw, Wt, x0, x1, lx);
    const long t00 = ((long)z0 * Ht + y0) * Wt, t01 = ((long)z0 * Ht + y1) * Wt;
    const long t10 = ((long)z1 * Ht + y0) * Wt, t11 = ((long)z1 * Ht + y1) * Wt;
    const float uz0 = 1.f - lz, uy0 = 1.f - ly, ux0 = 1.f - lx;
    u[0] = uz0 * uy0 * ux0; u[1] = uz0 * uy0 * lx; u[2] = uz0 * ly * ux0; u[3] = uz0 * ly * lx;
    u[4] = lz * uy0 * ux0; u[5] = lz * uy0 * lx; u[6] = lz * ly * ux0; u[7] = lz * ly * lx;
    tl[0] = load_label(tb, t00 + x0); tl[1] = load_label(tb, t00 + x1);
    tl[2] = load_label(tb, t01 + x0); tl[3] = load_label(tb, t01 + x1);
    tl[4] = load_label(tb, t10 + x0); tl[5] = load_label(tb, t10 + x1);
    tl[6] = load_label(tb, t11 + x0); tl[7] = load_label(tb, t11 + x1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (cl[i] < 0 || cl[i] >= C) cl[i] = -1;
        if (tl[i] < 0 || tl[i] >= C) tl[i] = -2;                 // (never equal to a corner's class, valid or not)
    }
    float G[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float pc = 0.f, tc = 0.f;                                 // matching weights added in corner / tap order, starting from 0, as the forward does
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            pc += cl[j] == cl[i] ? w[j] : 0.f;
            tc += tl[j] == cl[i] ? u[j] : 0.f;
        }
        const int c = cl[i] < 0 ? 0 : cl[i];
        const float g = tab[2 * c] * tc + tab[2 * c + 1] * pc;
        G[i] = cl[i] < 0 ? 0.f : g;
    }
    const float gz = (G[4] - G[0]) * (wy0 * wx0) + (G[5] - G[1]) * (wy0 * cx.f) + (G[6] - G[2]) * (cy.f * wx0) + (G[7] - G[3]) * (cy.f * cx.f);
    const float gy = (G[2] - G[0]) * (wz0 * wx0) + (G[3] - G[1]) * (wz0 * cx.f) + (G[6] - G[4]) * (cz.f * wx0) + (G[7] - G[5]) * (cz.f * cx.f);
    const float gx = (G[1] - G[0]) * (wz0 * wy0) + (G[3] - G[2]) * (wz0 * cy.f) + (G[5] - G[4]) * (cz.f * wy0) + (G[7] - G[6]) * (cz.f * cy.f);
    const float k0 = gup[0];
    float* o = ddf + (long)b * 3 * Vg + v;
    o[0] = k0 * cz.dscale * gz;
    o[Vg] = k0 * cy.dscale * gy;
    o[2 * Vg] = k0 * cx.dscale * gx;
}

// avg_pool3d(one_hot(labels), kernel 2, stride 2, ceil_mode) without the one-hot map: per output voxel the share of each class among the
// in-bounds voxels of its 2x2x2 window (1, 2, 4 or 8 of them: the values are counts over powers of two, exact).  grid (nblk, B); out planar
// (B, C, Do, Ho, Wo).  A label outside [0, C) counts for no class.
template <typename LT>
__global__ __launch_bounds__(256) void labels_pool2_kernel(const LT* __restrict__ lab, float* __restrict__ out, int C, int D, int H, int W, int Do,
                                                             int Ho, int Wo) {
    const int b = blockIdx.y;
    const long Vo = (long)Do * Ho * Wo;
    const LT* lb = lab + (long)b * D * H * W;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < Vo; v += (long)gridDim.x * 256) {
        const int vi = (int)v;
        const int ox = vi % Wo, oy = (vi / Wo) % Ho, oz = vi / (Wo * Ho);
        const int z0 = 2 * oz, y0 = 2 * oy, x0 = 2 * ox;
        const bool hz = z0 + 1 < D, hy = y0 + 1 < H, hx = x0 + 1 < W;
        const int z1 = hz ? z0 + 1 : z0, y1 = hy ? y0 + 1 : y0, x1 = hx ? x0 + 1 : x0;
        const long o00 = ((long)z0 * H + y0) * W, o01 = ((long)z0 * H + y1) * W, o10 = ((long)z1 * H + y0) * W, o11 = ((long)z1 * H + y1) * W;
        int cl[8];
        cl[0] = load_label(lb, o00 + x0);
        cl[1] = hx ? load_label(lb, o00 + x1) : -1;
        cl[2] = hy ? load_label(lb, o01 + x0) : -1;
        cl[3] = hy && hx ? load_label(lb, o01 + x1) : -1;
        cl[4] = hz ? load_label(lb, o10 + x0) : -1;
        cl[5] = hz && hx ? load_label(lb, o10 + x1) : -1;
        cl[6] = hz && hy ? load_label(lb, o11 + x0) : -1;
        cl[7] = hz && hy && hx ? load_label(lb, o11 + x1) : -1;
        const float inv = 1.f / (float)((hz ? 2 : 1) * (hy ? 2 : 1) * (hx ? 2 : 1));
        float* o = out + (long)b * C * Vo + v;
        for (int c = 0; c < C; ++c) {
            int n = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) n += cl[i] == c ? 1 : 0;
            o[(long)c * Vo] = (float)n * inv;
        }
    }
}

// F.interpolate(one_hot(labels), size, trilinear, align_corners=False) without the one-hot map: per output voxel and class the sum of the
// tap weights that carry the class - the taps, weights and summation order of t_c in warp_labels_soft_dice_kernel.  grid (nblk, B); out
// planar (B, C, Do, Ho, Wo).  A label outside [0, C) counts for no class.
template <typename LT>
__global__ __launch_bounds__(256) void labels_resize_kernel(const LT* __restrict__ lab, float* __restrict__ out, int C, int Dt, int Ht, int Wt, int Do,
                                                              int Ho, int Wo) {
    const int b = blockIdx.y;
    const long Vo = (long)Do * Ho * Wo;
    const LT* tb = lab + (long)b * Dt * Ht * Wt;
    const float sd = (float)Dt / (float)Do, shh = (float)Ht / (float)Ho, sw = (float)Wt / (float)Wo;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < Vo; v += (long)gridDim.x * 256) {
        const int vi = (int)v;
        const int x = vi % Wo, y = (vi / Wo) % Ho, z = vi / (Wo * Ho);
        int z0, z1, y0, y1, x0, x1;
        float lz, ly, lx;
        resize_src_index(z, sd, Dt, z0, z1, lz);
        resize_src_index(y, shh, Ht, y0, y1, ly);
        resize_src_index(x, sw, Wt, x0, x1, lx);
        const long t00 = ((long)z0 * Ht + y0) * Wt, t01 = ((long)z0 * Ht + y1) * Wt;
        const long t10 = ((long)z1 * Ht + y0) * Wt, t11 = ((long)z1 * Ht + y1) * Wt;
        const float uz0 = 1.f - lz, uy0 = 1.f - ly, ux0 = 1.f - lx;
        float u[8];
        int tl[8];
        u[0] = uz0 * uy0 * ux0; u[1] = uz0 * uy0 * lx; u[2] = uz0 * ly * ux0; u[3] = uz0 * ly * lx;
        u[4] = lz * uy0 * ux0; u[5] = lz * uy0 * lx; u[6] = lz * ly * ux0; u[7] = lz * ly * lx;
        tl[0] = load_label(tb, t00 + x0); tl[1] = load_label(tb, t00 + x1);
        tl[2] = load_label(tb, t01 + x0); tl[3] = load_label(tb, t01 + x1);
        tl[4] = load_label(tb, t10 + x0); tl[5] = load_label(tb, t10 + x1);
        tl[6] = load_label(tb, t11 + x0); tl[7] = load_label(tb, t11 + x1);
        float* o = out + (long)b * C * Vo + v;
        for (int c = 0; c < C; ++c) {
            float tc = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) tc += tl[i] == c ? u[i] : 0.f;
            o[(long)c * Vo] = tc;
        }
    }
}

}  // namespace

PULPO_API size_t pulpo_warp_labels_ws_bytes(int B, int C) { return sizeof(unsigned long long) * 3 * (size_t)std::max(B, 0) * std::max(C, 0); }

PULPO_API int pulpo_warp_labels(const float* df, const void* labels, int ldt, int C, const void* target, float* onehot, void* amax, float* dice,
                                float* mean, float* m2, int k, void* ws, int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi,
                                void* stream) {
    PULPO_REQUIRE(df && labels && flag && B > 0 && (ldt == 0 || ldt == 1) && C >= 1 && C <= kMaxClasses, "warp_labels: bad arguments (1 <= C <= 256)");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && (Dg > 1 || Di == 1),
                  "warp_labels: grid H, W must be > 1 (depth 1 = 2-D form, with a depth-1 label map)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "warp_labels: grids of 2^31 voxels and more are not supported");
    PULPO_REQUIRE((target == nullptr) == (dice == nullptr) && (target == nullptr || ws != nullptr), "warp_labels: target, dice and ws go together");
    PULPO_REQUIRE((mean == nullptr) == (m2 == nullptr) && (mean == nullptr || k >= 1), "warp_labels: mean and m2 go together (k >= 1)");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e == hipSuccess && target != nullptr) e = hipMemsetAsync(ws, 0, pulpo_warp_labels_ws_bytes(B, C), st);
    if (e != hipSuccess) return pulpo::fail((int)e, "warp_labels memset: %s", hipGetErrorString(e));
    const long Vg = (long)Dg * Hg * Wg;
    const dim3 grid(eblocks(Vg, std::max(1, 2048 / B)), B);
    unsigned long long* sums = (unsigned long long*)ws;
    if (ldt == 0)
        hipLaunchKernelGGL(warp_labels_kernel<uint8_t>, grid, dim3(256), 0, st, df, (const uint8_t*)labels, C, (const uint8_t*)target, onehot,
                           (uint8_t*)amax, mean, m2, k, sums, flag, Dg, Hg, Wg, Di, Hi, Wi);
    else
        hipLaunchKernelGGL(warp_labels_kernel<int32_t>, grid, dim3(256), 0, st, df, (const int32_t*)labels, C, (const int32_t*)target, onehot,
                           (int32_t*)amax, mean, m2, k, sums, flag, Dg, Hg, Wg, Di, Hi, Wi);
    int rc = pulpo::check_launch("warp_labels");
    if (rc || target == nullptr) return rc;
    const int n = B * C;
    hipLaunchKernelGGL(dice_from_sums_kernel, dim3((n + 255) / 256), dim3(256), 0, st, sums, n, (double)Vg, dice);
    return pulpo::check_launch("warp_labels dice");
}

PULPO_API int pulpo_warp_labels_soft_dice(const float* df, const void* labels, const void* target, int ldt, int C, float* dice, float* mean, void* ws,
                                          int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt, void* stream) {
    PULPO_REQUIRE(df && labels && target && dice && mean && ws && flag && B > 0 && (ldt == 0 || ldt == 1) && C >= 1 && C <= kMaxClasses,
                  "warp_labels_soft_dice: bad arguments (1 <= C <= 256)");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && Dt > 0 && Ht > 0 && Wt > 0 && (Dg > 1 || (Di == 1 && Dt == 1)),
                  "warp_labels_soft_dice: grid H, W must be > 1 (depth 1 = 2-D form, with depth-1 label maps)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "warp_labels_soft_dice: grids of 2^31 voxels and more are not supported");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(ws, 0, pulpo_warp_labels_ws_bytes(B, C), st);
    if (e != hipSuccess) return pulpo::fail((int)e, "warp_labels_soft_dice memset: %s", hipGetErrorString(e));
    const long Vg = (long)Dg * Hg * Wg;
    const dim3 grid(eblocks(Vg, std::max(1, 2048 / B)), B);
    unsigned long long* sums = (unsigned long long*)ws;
    if (ldt == 0)
        hipLaunchKernelGGL(warp_labels_soft_dice_kernel<uint8_t>, grid, dim3(256), 0, st, df, (const uint8_t*)labels, (const uint8_t*)target, C, sums,
                           flag, Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    else
        hipLaunchKernelGGL(warp_labels_soft_dice_kernel<int32_t>, grid, dim3(256), 0, st, df, (const int32_t*)labels, (const int32_t*)target, C, sums,
                           flag, Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    int rc = pulpo::check_launch("warp_labels_soft_dice");
    if (rc) return rc;
    hipLaunchKernelGGL(soft_dice_from_sums_kernel, dim3(1), dim3(64), 0, st, sums, B * C, dice, mean);
    return pulpo::check_launch("warp_labels_soft_dice finish");
}

// The Dice term of the training step from label maps: the sums of pulpo_warp_labels_soft_dice, finished into the loss,
// the per-class Dice and the (B, C, 2) coefficient table of pulpo_label_dice_bwd
PULPO_API int pulpo_label_dice_fwd(const float* df, const void* labels, const void* target, int ldt, int C, float dice_factor, float* loss, float* dice,
                                   float* coef, void* ws, int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt,
                                   void* stream) {
    PULPO_REQUIRE(df && labels && target && loss && dice && coef && ws && flag && B > 0 && B <= 65535 && (ldt == 0 || ldt == 1) && C >= 1 &&
                      C <= kMaxClasses && dice_factor != 0.f,
                  "label_dice_fwd: bad arguments (1 <= C <= 256, B <= 65535)");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && Dt > 0 && Ht > 0 && Wt > 0 && (Dg > 1 || (Di == 1 && Dt == 1)),
                  "label_dice_fwd: grid H, W must be > 1 (depth 1 = 2-D form, with depth-1 label maps)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "label_dice_fwd: grids of 2^31 voxels and more are not supported");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(ws, 0, pulpo_warp_labels_ws_bytes(B, C), st);
    if (e != hipSuccess) return pulpo::fail((int)e, "label_dice_fwd memset: %s", hipGetErrorString(e));
    const long Vg = (long)Dg * Hg * Wg;
    const dim3 grid(eblocks(Vg, std::max(1, 2048 / B)), B);
    unsigned long long* sums = (unsigned long long*)ws;
    if (ldt == 0)
        hipLaunchKernelGGL(warp_labels_soft_dice_kernel<uint8_t>, grid, dim3(256), 0, st, df, (const uint8_t*)labels, (const uint8_t*)target, C, sums,
                           flag, Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    else
        hipLaunchKernelGGL(warp_labels_soft_dice_kernel<int32_t>, grid, dim3(256), 0, st, df, (const int32_t*)labels, (const int32_t*)target, C, sums,
                           flag, Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    int rc = pulpo::check_launch("label_dice_fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(label_dice_finish_kernel, dim3(1), dim3(64), 0, st, sums, B * C, (double)Vg / (double)dice_factor, dice, coef, loss);
    return pulpo::check_launch("label_dice_fwd finish");
}

PULPO_API int pulpo_label_dice_bwd(const float* df, const void* labels, const void* target, int ldt, int C, const float* coef, const float* gup,
                                   float* ddf, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt, void* stream) {
    PULPO_REQUIRE(df && labels && target && coef && gup && ddf && B > 0 && B <= 65535 && (ldt == 0 || ldt == 1) && C >= 1 && C <= kMaxClasses,
                  "label_dice_bwd: bad arguments (1 <= C <= 256, B <= 65535)");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && Dt > 0 && Ht > 0 && Wt > 0 && (Dg > 1 || (Di == 1 && Dt == 1)),
                  "label_dice_bwd: grid H, W must be > 1 (depth 1 = 2-D form, with depth-1 label maps)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "label_dice_bwd: grids of 2^31 voxels and more are not supported");
    hipStream_t st = (hipStream_t)stream;
    const long Vg = (long)Dg * Hg * Wg;
    const dim3 grid((unsigned)((Vg + 255) / 256), B);
    if (ldt == 0)
        hipLaunchKernelGGL(label_dice_bwd_kernel<uint8_t>, grid, dim3(256), 0, st, df, (const uint8_t*)labels, (const uint8_t*)target, C, coef, gup, ddf,
                           Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    else
        hipLaunchKernelGGL(label_dice_bwd_kernel<int32_t>, grid, dim3(256), 0, st, df, (const int32_t*)labels, (const int32_t*)target, C, coef, gup, ddf,
                           Dg, Hg, Wg, Di, Hi, Wi, Dt, Ht, Wt);
    return pulpo::check_launch("label_dice_bwd");
}

PULPO_API int pulpo_labels_pool2(const void* labels, int ldt, int C, float* out, int B, int D, int H, int W, void* stream) {
    PULPO_REQUIRE(labels && out && B > 0 && B <= 65535 && (ldt == 0 || ldt == 1) && C >= 1 && D > 0 && H > 0 && W > 0, "labels_pool2: bad arguments");
    PULPO_REQUIRE((long)D * H * W < (1L << 31), "labels_pool2: maps of 2^31 voxels and more are not supported");
    const int Do = (D + 1) / 2, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const dim3 grid(eblocks((long)Do * Ho * Wo, std::max(1, 4096 / B)), B);
    hipStream_t st = (hipStream_t)stream;
    if (ldt == 0) hipLaunchKernelGGL(labels_pool2_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)labels, out, C, D, H, W, Do, Ho, Wo);
    else hipLaunchKernelGGL(labels_pool2_kernel<int32_t>, grid, dim3(256), 0, st, (const int32_t*)labels, out, C, D, H, W, Do, Ho, Wo);
    return pulpo::check_launch("labels_pool2");
}

PULPO_API int pulpo_labels_resize(const void* labels, int ldt, int C, float* out, int B, int Dt, int Ht, int Wt, int Do, int Ho, int Wo, void* stream) {
    PULPO_REQUIRE(labels && out && B > 0 && B <= 65535 && (ldt == 0 || ldt == 1) && C >= 1 && Dt > 0 && Ht > 0 && Wt > 0 && Do > 0 && Ho > 0 && Wo > 0,
                  "labels_resize: bad arguments");
    PULPO_REQUIRE((long)Do * Ho * Wo < (1L << 31), "labels_resize: outputs of 2^31 voxels and more are not supported");
    const dim3 grid(eblocks((long)Do * Ho * Wo, std::max(1, 4096 / B)), B);
    hipStream_t st = (hipStream_t)stream;
    if (ldt == 0) hipLaunchKernelGGL(labels_resize_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)labels, out, C, Dt, Ht, Wt, Do, Ho, Wo);
    else hipLaunchKernelGGL(labels_resize_kernel<int32_t>, grid, dim3(256), 0, st, (const int32_t*)labels, out, C, Dt, Ht, Wt, Do, Ho, Wo);
    return pulpo::check_launch("labels_resize");
}

PULPO_API int pulpo_labels_check(const void* labels, int ldt, int64_t n, int C, int* flag, void* stream) {
    PULPO_REQUIRE(labels && flag && n > 0 && (ldt == 0 || ldt == 1), "labels_check: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e != hipSuccess) return pulpo::fail((int)e, "labels_check memset: %s", hipGetErrorString(e));
    if (ldt == 0) hipLaunchKernelGGL(labels_check_kernel<uint8_t>, dim3(eblocks(n, 2048)), dim3(256), 0, st, (const uint8_t*)labels, (long)n, C, flag);
    else hipLaunchKernelGGL(labels_check_kernel<int32_t>, dim3(eblocks(n, 2048)), dim3(256), 0, st, (const int32_t*)labels, (long)n, C, flag);
    return pulpo::check_launch("labels_check");
}

PULPO_API int pulpo_labels_from_onehot(const float* seg, void* labels, int ldt, int B, int C, int64_t V, void* stream) {
    PULPO_REQUIRE(seg && labels && B > 0 && C >= 1 && V > 0 && (ldt == 1 || (ldt == 0 && C <= 256)), "labels_from_onehot: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)B * V;
    if (ldt == 0) hipLaunchKernelGGL(labels_from_onehot_kernel<uint8_t>, dim3(eblocks(total, 4096)), dim3(256), 0, st, seg, (uint8_t*)labels, C, (long)V, total);
    else hipLaunchKernelGGL(labels_from_onehot_kernel<int32_t>, dim3(eblocks(total, 4096)), dim3(256), 0, st, seg, (int32_t*)labels, C, (long)V, total);
    return pulpo::check_launch("labels_from_onehot");
}

PULPO_API int pulpo_map_ncc_blocks(int64_t n) { return eblocks(n, 1024); }

PULPO_API int pulpo_map_ncc(const float* a, const float* b, int64_t n, double* partial, double* out, void* stream) {
    PULPO_REQUIRE(a && b && partial && out && n > 0, "map_ncc: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = pulpo_map_ncc_blocks(n);
    double* part2 = partial + 2 * nblk;
    hipLaunchKernelGGL(ncc_sums_kernel, dim3(nblk), dim3(256), 0, st, a, b, (long)n, partial);
    int rc = pulpo::check_launch("map_ncc sums");
    if (rc) return rc;
    hipLaunchKernelGGL(ncc_centred_kernel, dim3(nblk), dim3(256), 0, st, a, b, (long)n, partial, part2);
    rc = pulpo::check_launch("map_ncc centred");
    if (rc) return rc;
    hipLaunchKernelGGL(ncc_finalize_kernel, dim3(1), dim3(64), 0, st, part2, nblk, (long)n, out);
    return pulpo::check_launch("map_ncc finalize");
}
