// Cubic B-spline interpolation of the final resample: the recursive prefilter that turns samples into interpolating
// coefficients, the 64-tap gather at the deformable warp's sample coordinate, and the gather's gradient with respect to the field.
// No reference counterpart: the reference's SpatialTransformer stores its `mode` and resamples trilinearly.  The definition is
// scipy.ndimage's order-3 spline with mode="mirror" (spline_filter / map_coordinates) at pulpo::sample_coord's clamped coordinate.
//   prefilter  per axis of N >= 2 samples: c+[k] = 6 s[k] + z c+[k-1], c[k] = z (c[k+1] - c+[k]), z = sqrt(3) - 2, with the mirror starts of
//              cubic_core.h.  One thread owns one line.  Along D and H neighbouring threads are neighbours along W (coalesced) and walk memory
//              directly; along W 64 lines go through a 64-column LDS tile (row stride 65 dwords: the 32 lanes of a half wave walking their own
//              rows sit on 32 different banks), the recursion carried from chunk to chunk, so a line of any length is exact.
//   gather     one thread per output voxel: coordinate, four weights and four mirrored taps per axis once, shared by the channels; 64 loads
//              per channel served by L1 / L2.  The field gradient is the same gather with the derivative weights: no scatter, no atomics -
//              deterministic by construction.  The image gradient is not built (the image is data).
#include "common.h"
#include "cubic_core.h"
#include "sampling.h"

namespace {

using pulpo::Corner;
using pulpo::cubic_anticausal_start;
using pulpo::cubic_causal_start;
using pulpo::cubic_dweights;
using pulpo::cubic_taps;
using pulpo::cubic_weights;
using pulpo::kCubicGain;
using pulpo::kCubicPole;
using pulpo::sample_coord;

constexpr int kLines = 64;             // lines per workgroup (one wave: a lane per line)
constexpr int kTile = 64;              // columns per LDS chunk of the W pass
constexpr int kTileStride = kTile + 1; // odd: lane t's row starts at bank t mod 32

// One axis whose samples lie `inner` elements apart (D: inner = H W; H: inner = W): line L = (o, r) starts at o N inner + r.  src may be dst
// (each thread reads an element of its line before it writes it), so neither is __restrict__.
__global__ __launch_bounds__(kLines) void prefilter_strided_kernel(const float* src, float* dst, long nlines, int N, long inner) {
    const long L = blockIdx.x * (long)kLines + threadIdx.x;
    if (L >= nlines) return;
    const long o = L / inner, base = o * N * inner + (L - o * inner);
    const float* s = src + base;
    float* d = dst + base;
    const float z = kCubicPole;
    float cp = cubic_causal_start([&](int k) { return kCubicGain * s[k * inner]; }, N), cp_prev = cp;
    d[0] = cp;
    int k = 1;
    for (; k + 8 <= N; k += 8) {                       // eight independent loads in flight per trip; the recursion itself is eight FMAs
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s[(k + j) * inner];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            cp_prev = cp;
            cp = __fmaf_rn(z, cp, kCubicGain * v[j]);
            d[(k + j) * inner] = cp;
        }
    }
    for (; k < N; ++k) {
        cp_prev = cp;
        cp = __fmaf_rn(z, cp, kCubicGain * s[k * inner]);
        d[k * inner] = cp;
    }
    float c = cubic_anticausal_start(cp, cp_prev);
    d[(long)(N - 1) * inner] = c;
    k = N - 2;
    for (; k >= 7; k -= 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = d[(k - j) * inner];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c = z * (c - v[j]);
            d[(k - j) * inner] = c;
        }
    }
    for (; k >= 0; --k) {
        c = z * (c - d[k * inner]);
        d[k * inner] = c;
    }
}

// The W axis (contiguous lines of N samples): kLines lines per workgroup, kTile columns at a time through LDS.  Forward over the chunks
// (causal values written to dst; the last chunk is finished in LDS), then back over the earlier chunks reading the causal values again.
__global__ __launch_bounds__(kLines) void prefilter_rows_kernel(const float* src, float* dst, long nlines, int N) {
    __shared__ float tile[kLines * kTileStride];
    const int t = threadIdx.x;
    const long l0 = blockIdx.x * (long)kLines;
    const int nl = (int)((nlines - l0) < (long)kLines ? (nlines - l0) : (long)kLines);
    const int nchunks = (N + kTile - 1) / kTile;
    const float z = kCubicPole;
    float* row = tile + t * kTileStride;
    float cp = 0.f, cp_prev = 0.f, c = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * kTile, cw = (N - c0) < kTile ? (N - c0) : kTile;
        if (t < cw) {
#pragma unroll 8
            for (int r = 0; r < nl; ++r) tile[r * kTileStride + t] = kCubicGain * src[(l0 + r) * N + c0 + t];
        }
        __syncthreads();
        if (t < nl) {
            int k = 0;
            if (ch == 0) {                              // (min(N, kCubicHorizon) <= cw: the start sum reads this chunk only)
                cp = cubic_causal_start([&](int q) { return row[q]; }, N);
                cp_prev = cp;
                row[0] = cp;
                k = 1;
            }
            for (; k < cw; ++k) {
                cp_prev = cp;
                cp = __fmaf_rn(z, cp, row[k]);
                row[k] = cp;
            }
            if (ch == nchunks - 1) {
                c = cubic_anticausal_start(cp, cp_prev);
                row[cw - 1] = c;
                for (k = cw - 2; k >= 0; --k) {
                    c = z * (c - row[k]);
                    row[k] = c;
                }
            }
        }
        __syncthreads();
        if (t < cw) {
#pragma unroll 8
            for (int r = 0; r < nl; ++r) dst[(l0 + r) * N + c0 + t] = tile[r * kTileStride + t];
        }
        __syncthreads();
    }
    for (int ch = nchunks - 2; ch >= 0; --ch) {         // (every earlier chunk is full)
        const int c0 = ch * kTile;
#pragma unroll 8
        for (int r = 0; r < nl; ++r) tile[r * kTileStride + t] = dst[(l0 + r) * N + c0 + t];
        __syncthreads();
        if (t < nl) {
            for (int k = kTile - 1; k >= 0; --k) {
                c = z * (c - row[k]);
                row[k] = c;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < nl; ++r) dst[(l0 + r) * N + c0 + t] = tile[r * kTileStride + t];
        __syncthreads();
    }
}

// the coordinate, weights and taps of one output voxel, shared by the channels
struct CubicSite {
    float wz[4], wy[4], wx[4];
    int tz[4], ty[4], tx[4];
    Corner cz, cy, cx;
};

__device__ __forceinline__ void cubic_site(CubicSite& S, const float* __restrict__ d, long Vg, int z, int y, int x, int Dg, int Hg, int Wg, int Di,
                                           int Hi, int Wi) {
    S.cz = sample_coord((float)z, d[0], Dg, Di);
    S.cy = sample_coord((float)y, d[Vg], Hg, Hi);
    S.cx = sample_coord((float)x, d[2 * Vg], Wg, Wi);
    cubic_weights(S.cz.f, Dg == 1, S.wz);
    cubic_weights(S.cy.f, Hg == 1, S.wy);
    cubic_weights(S.cx.f, Wg == 1, S.wx);
    cubic_taps(S.cz.i0, Di, Dg == 1, S.tz);
    cubic_taps(S.cy.i0, Hi, Hg == 1, S.ty);
    cubic_taps(S.cx.i0, Wi, Wg == 1, S.tx);
}

// out[b][c][v] = sum over the 4 x 4 x 4 taps of B(fz) B(fy) B(fx) coef[b][c][m(tap)];  NZ = 1: a depth-1 grid (one depth tap of weight 1)
template <int NZ>
__global__ __launch_bounds__(256) void warp_cubic_fwd_kernel(const float* __restrict__ df, const float* __restrict__ coef, float* __restrict__ out, int B,
                                                               int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi) {
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi;
    const long total = (long)B * Vg;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long b = B == 1 ? 0 : e / Vg, v = e - b * Vg;
        const int vi = (int)v;
        const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
        CubicSite S;
        cubic_site(S, df + b * 3 * Vg + v, Vg, z, y, x, Dg, Hg, Wg, Di, Hi, Wi);
        for (int c = 0; c < C; ++c) {
            const float* s = coef + (b * C + c) * Vi;
            float acc = 0.f;
#pragma unroll
            for (int l = 0; l < NZ; ++l)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float* r = s + ((long)S.tz[l] * Hi + S.ty[m]) * Wi;
                    const float rv = __fmaf_rn(S.wx[3], r[S.tx[3]], __fmaf_rn(S.wx[2], r[S.tx[2]], __fmaf_rn(S.wx[1], r[S.tx[1]], S.wx[0] * r[S.tx[0]])));
                    acc = __fmaf_rn(S.wz[l] * S.wy[m], rv, acc);
                }
            out[(b * C + c) * Vg + v] = acc;
        }
    }
}

// gdf[b][a][v] = dscale_a sum_c g[b][c][v] sum over the taps of B'(f_a) B(f_b) B(f_c) coef[b][c][m(tap)]: plain stores, every element written
template <int NZ>
__global__ __launch_bounds__(256) void warp_cubic_bwd_kernel(const float* __restrict__ df, const float* __restrict__ coef, const float* __restrict__ gout,
                                                               float* __restrict__ gdf, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi) {
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi;
    const long total = (long)B * Vg;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long b = B == 1 ? 0 : e / Vg, v = e - b * Vg;
        const int vi = (int)v;
        const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
        CubicSite S;
        cubic_site(S, df + b * 3 * Vg + v, Vg, z, y, x, Dg, Hg, Wg, Di, Hi, Wi);
        float dz[4], dy[4], dx[4];
        cubic_dweights(S.cz.f, Dg == 1, dz);
        cubic_dweights(S.cy.f, Hg == 1, dy);
        cubic_dweights(S.cx.f, Wg == 1, dx);
        float gz = 0.f, gy = 0.f, gx = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* s = coef + (b * C + c) * Vi;
            float az = 0.f, ay = 0.f, ax = 0.f;
#pragma unroll
            for (int l = 0; l < NZ; ++l)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float* r = s + ((long)S.tz[l] * Hi + S.ty[m]) * Wi;
                    const float s0 = r[S.tx[0]], s1 = r[S.tx[1]], s2 = r[S.tx[2]], s3 = r[S.tx[3]];
                    const float rv = __fmaf_rn(S.wx[3], s3, __fmaf_rn(S.wx[2], s2, __fmaf_rn(S.wx[1], s1, S.wx[0] * s0)));
                    const float rd = __fmaf_rn(dx[3], s3, __fmaf_rn(dx[2], s2, __fmaf_rn(dx[1], s1, dx[0] * s0)));
                    az = __fmaf_rn(dz[l] * S.wy[m], rv, az);
                    ay = __fmaf_rn(S.wz[l] * dy[m], rv, ay);
                    ax = __fmaf_rn(S.wz[l] * S.wy[m], rd, ax);
                }
            const float g = gout[(b * C + c) * Vg + v];
            gz = __fmaf_rn(g, az, gz);
            gy = __fmaf_rn(g, ay, gy);
            gx = __fmaf_rn(g, ax, gx);
        }
        float* q = gdf + b * 3 * Vg + v;
        q[0] = gz * S.cz.dscale;
        q[Vg] = gy * S.cy.dscale;
        q[2 * Vg] = gx * S.cx.dscale;
    }
}

}  // namespace

// img, coef: `planes` volumes (D,H,W), planar fp32; coef may not be img.  Axes of one sample are left alone.
PULPO_API int pulpo_bspline_prefilter(const float* img, float* coef, int planes, int D, int H, int W, void* stream) {
    PULPO_REQUIRE(img && coef && img != coef && planes > 0 && D > 0 && H > 0 && W > 0, "bspline_prefilter: bad arguments (out of place, extents >= 1)");
    PULPO_REQUIRE((long)D * H * W < (1L << 31), "bspline_prefilter: volumes of 2^31 voxels and more are not supported");
    hipStream_t st = (hipStream_t)stream;
    const long V = (long)D * H * W;
    const float* src = img;
    if (W > 1) {
        const long nlines = (long)planes * D * H;
        hipLaunchKernelGGL(prefilter_rows_kernel, dim3(pulpo::cdiv(nlines, kLines)), dim3(kLines), 0, st, src, coef, nlines, W);
        src = coef;
    }
    if (H > 1) {
        const long nlines = (long)planes * D * W;
        hipLaunchKernelGGL(prefilter_strided_kernel, dim3(pulpo::cdiv(nlines, kLines)), dim3(kLines), 0, st, src, coef, nlines, H, (long)W);
        src = coef;
    }
    if (D > 1) {
        const long nlines = (long)planes * H * W;
        hipLaunchKernelGGL(prefilter_strided_kernel, dim3(pulpo::cdiv(nlines, kLines)), dim3(kLines), 0, st, src, coef, nlines, D, (long)H * W);
        src = coef;
    }
    if (src == img) {                                   // a single sample per plane: its own coefficient
        hipError_t e = hipMemcpyAsync(coef, img, sizeof(float) * (size_t)planes * V, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return pulpo::fail((int)e, "bspline_prefilter copy: %s", hipGetErrorString(e));
    }
    return pulpo::check_launch("bspline_prefilter");
}

// df: (B,3,Dg,Hg,Wg) planar; coef: (B,C,Di,Hi,Wi) planar (pulpo_bspline_prefilter of the image); out: (B,C,Dg,Hg,Wg)
PULPO_API int pulpo_warp3d_cubic_fwd(const float* df, const float* coef, float* out, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi,
                                     void* stream) {
    PULPO_REQUIRE(df && coef && out && B > 0 && C > 0, "warp3d_cubic_fwd: bad arguments");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && (Dg > 1 || Di == 1), "warp3d_cubic_fwd: grid H, W must be > 1 (depth 1 = 2-D form, with a depth-1 image)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31) && (long)Di * Hi * Wi < (1L << 31), "warp3d_cubic_fwd: grids of 2^31 voxels and more are not supported");
    const long total = (long)B * Dg * Hg * Wg;
    hipStream_t st = (hipStream_t)stream;
    if (Dg == 1) hipLaunchKernelGGL(warp_cubic_fwd_kernel<1>, dim3(pulpo::eblocks(total, 8192)), dim3(256), 0, st, df, coef, out, B, C, Dg, Hg, Wg, Di, Hi, Wi);
    else hipLaunchKernelGGL(warp_cubic_fwd_kernel<4>, dim3(pulpo::eblocks(total, 8192)), dim3(256), 0, st, df, coef, out, B, C, Dg, Hg, Wg, Di, Hi, Wi);
    return pulpo::check_launch("warp3d_cubic_fwd");
}

// gdf: (B,3,grid) written (every element; the depth component of a depth-1 grid is 0)
PULPO_API int pulpo_warp3d_cubic_bwd(const float* df, const float* coef, const float* gout, float* gdf, int B, int C, int Dg, int Hg, int Wg, int Di,
                                     int Hi, int Wi, void* stream) {
    PULPO_REQUIRE(df && coef && gout && gdf && B > 0 && C > 0, "warp3d_cubic_bwd: bad arguments");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di > 0 && Hi > 0 && Wi > 0 && (Dg > 1 || Di == 1), "warp3d_cubic_bwd: grid H, W must be > 1 (depth 1 = 2-D form, with a depth-1 image)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31) && (long)Di * Hi * Wi < (1L << 31), "warp3d_cubic_bwd: grids of 2^31 voxels and more are not supported");
    const long total = (long)B * Dg * Hg * Wg;
    hipStream_t st = (hipStream_t)stream;
    if (Dg == 1) hipLaunchKernelGGL(warp_cubic_bwd_kernel<1>, dim3(pulpo::eblocks(total, 8192)), dim3(256), 0, st, df, coef, gout, gdf, B, C, Dg, Hg, Wg, Di, Hi, Wi);
    else hipLaunchKernelGGL(warp_cubic_bwd_kernel<4>, dim3(pulpo::eblocks(total, 8192)), dim3(256), 0, st, df, coef, gout, gdf, B, C, Dg, Hg, Wg, Di, Hi, Wi);
    return pulpo::check_launch("warp3d_cubic_bwd");
}
