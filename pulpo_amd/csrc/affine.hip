// Affine pre-alignment: the affine transform as a device operator.
//   pulpo_affine_field        the displacement field d(v) = p(v) - v an affine stands for: the bridge to every operator that takes a field.
//   pulpo_affine_warp_fwd     warp3d(affine_field(theta), img) without the field: reads the image, writes the result (8 bytes per voxel and
//                             channel against 32 for field + warp); bit-identical to pulpo_warp3d_fwd on the materialised field.
//   pulpo_affine_warp_bwd     the gradient with respect to the twelve entries of theta (the image is data): per-thread sums in double over a
//                             grid-stride loop, wave shuffles, LDS, one row of 12 doubles per block; a second launch adds the rows in a fixed
//                             order.  No float atomics: the same bits on every call.
//   pulpo_affine_compose      "affine first, deformable second" as one field on the deformable field's grid.
// theta: (B,3,4) fp32 [M | t] in voxel units of a stated grid about its centre (affine_core.h); a depth-1 grid is the 2-D form, with an
// identity depth row.  Gather kernels bound by latency and bytes like warp.hip's: one thread per output voxel, lanes along x, the batch
// element in blockIdx.y so that theta's twelve values are uniform over the block.
#include "common.h"
#include "affine_core.h"
#include "sampling.h"

extern "C" int pulpo_loss_blocks(int64_t n);

namespace {

using pulpo::Affine;
using pulpo::affine_disp;
using pulpo::affine_load;
using pulpo::affine_pos;
using pulpo::Corner;
using pulpo::sample_coord;

// out[b][a][v] = d_a(v); VEC consecutive voxels of a row per thread (VEC = 4: rows of a multiple of 4 voxels, 16-byte aligned planes)
template <int VEC>
__global__ __launch_bounds__(256) void affine_field_kernel(const float* __restrict__ theta, float* __restrict__ out, int D, int H, int W) {
    const int b = blockIdx.y;
    const Affine A = affine_load(theta + (long)b * 12, D, H, W);
    const long V = (long)D * H * W, n = V / VEC;
    float* o = out + (long)b * 3 * V;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int vi = (int)(e * VEC);
        const int x = vi % W, y = (vi / W) % H, z = vi / (W * H);
        float r[3][VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float d[3];
            affine_disp(A, (float)z, (float)y, (float)(x + k), d);
            r[0][k] = D == 1 ? 0.f : d[0];           // (the 2-D form has no depth displacement, whatever theta's depth row holds)
            r[1][k] = d[1];
            r[2][k] = d[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(o + a * V + vi) = make_float4(r[a][0], r[a][1], r[a][2], r[a][3]);
            else o[a * V + vi] = r[a][0];
        }
    }
}

// out[b][c][v] = trilinear(img[b][c], grid position v displaced by d(v)): warp_fwd_kernel's coordinate, corners and interpolation expression
// (warp.hip), the displacement formed here instead of read
template <int C>
__global__ __launch_bounds__(256) void affine_warp_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ img, float* __restrict__ out,
                                                                int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Cr) {
    const int b = blockIdx.y;
    const Affine A = affine_load(theta + (long)b * 12, Dg, Hg, Wg);
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi;
    const int nch = C > 0 ? C : Cr;
    // One voxel per thread, no grid-stride loop: with a loop the compiler kept two versions of the body, and the one a capped grid ran packed
    // the coordinate arithmetic of neighbouring trips (v_pk_fma_f32) - a quarter of the voxels then differed from pulpo_warp3d_fwd in the
    // last bit at 132^3 and above, where the straight-line body agrees with it bit for bit (tests/test_gpu_affine.py holds both sizes).
    const long v = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (v < Vg) {
        const int vi = (int)v;
        const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
        float d[3];
        affine_disp(A, (float)z, (float)y, (float)x, d);
        const Corner cz = sample_coord((float)z, d[0], Dg, Di);
        const Corner cy = sample_coord((float)y, d[1], Hg, Hi);
        const Corner cx = sample_coord((float)x, d[2], Wg, Wi);
        const long o00 = ((long)cz.i0 * Hi + cy.i0) * Wi, o01 = ((long)cz.i0 * Hi + cy.i1) * Wi;
        const long o10 = ((long)cz.i1 * Hi + cy.i0) * Wi, o11 = ((long)cz.i1 * Hi + cy.i1) * Wi;
        const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
        for (int c = 0; c < nch; ++c) {
            const float* s = img + ((long)b * nch + c) * Vi;
            float val = wz0 * wy0 * wx0 * s[o00 + cx.i0] + wz0 * wy0 * cx.f * s[o00 + cx.i1] + wz0 * cy.f * wx0 * s[o01 + cx.i0] +
                        wz0 * cy.f * cx.f * s[o01 + cx.i1] + cz.f * wy0 * wx0 * s[o10 + cx.i0] + cz.f * wy0 * cx.f * s[o10 + cx.i1] +
                        cz.f * cy.f * wx0 * s[o11 + cx.i0] + cz.f * cy.f * cx.f * s[o11 + cx.i1];
            out[((long)b * nch + c) * Vg + v] = val;
        }
    }
}

// Block (blockIdx.x, b) -> ws[(b * gridDim.x + blockIdx.x) * 12 + k], k = 4 a + j: the block's share of
//   gtheta[a][j] = sum_v gpos_a (v_j - c_j)  (j < 3),  gtheta[a][3] = sum_v gpos_a,
// gpos_a = dscale_a * sum_c gout_c * d interp / d coord_a, warp_bwd_kernel's displacement gradient (warp.hip) in its fp32 expression;
// the products with v - c and the sums in double.
__global__ __launch_bounds__(256) void affine_warp_bwd_kernel(const float* __restrict__ theta, const float* __restrict__ img, const float* __restrict__ gout,
                                                                double* __restrict__ ws, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int nch) {
    __shared__ double sh[4][12];
    const int b = blockIdx.y;
    const Affine A = affine_load(theta + (long)b * 12, Dg, Hg, Wg);
    const long Vg = (long)Dg * Hg * Wg, Vi = (long)Di * Hi * Wi;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < Vg; v += (long)gridDim.x * blockDim.x) {
        const int vi = (int)v;
        const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
        float d[3];
        affine_disp(A, (float)z, (float)y, (float)x, d);
        const Corner cz = sample_coord((float)z, d[0], Dg, Di);
        const Corner cy = sample_coord((float)y, d[1], Hg, Hi);
        const Corner cx = sample_coord((float)x, d[2], Wg, Wi);
        const long o00 = ((long)cz.i0 * Hi + cy.i0) * Wi, o01 = ((long)cz.i0 * Hi + cy.i1) * Wi;
        const long o10 = ((long)cz.i1 * Hi + cy.i0) * Wi, o11 = ((long)cz.i1 * Hi + cy.i1) * Wi;
        const float wz0 = 1.f - cz.f, wy0 = 1.f - cy.f, wx0 = 1.f - cx.f;
        float gz = 0.f, gy = 0.f, gx = 0.f;
        for (int c = 0; c < nch; ++c) {
            const float g = gout[((long)b * nch + c) * Vg + v];
            const float* s = img + ((long)b * nch + c) * Vi;
            const float s000 = s[o00 + cx.i0], s001 = s[o00 + cx.i1], s010 = s[o01 + cx.i0], s011 = s[o01 + cx.i1];
            const float s100 = s[o10 + cx.i0], s101 = s[o10 + cx.i1], s110 = s[o11 + cx.i0], s111 = s[o11 + cx.i1];
            gz += g * (wy0 * wx0 * (s100 - s000) + wy0 * cx.f * (s101 - s001) + cy.f * wx0 * (s110 - s010) + cy.f * cx.f * (s111 - s011));
            gy += g * (wz0 * wx0 * (s010 - s000) + wz0 * cx.f * (s011 - s001) + cz.f * wx0 * (s110 - s100) + cz.f * cx.f * (s111 - s101));
            gx += g * (wz0 * wy0 * (s001 - s000) + wz0 * cy.f * (s011 - s010) + cz.f * wy0 * (s101 - s100) + cz.f * cy.f * (s111 - s110));
        }
        const double gp[3] = {(double)(gz * cz.dscale), (double)(gy * cy.dscale), (double)(gx * cx.dscale)};
        const double uz = (double)((float)z - A.cz), uy = (double)((float)y - A.cy), ux = (double)((float)x - A.cx);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[4 * a] += gp[a] * uz;
            acc[4 * a + 1] += gp[a] * uy;
            acc[4 * a + 2] += gp[a] * ux;
            acc[4 * a + 3] += gp[a];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double s = pulpo::wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;
        ws[((long)b * gridDim.x + blockIdx.x) * 12 + k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
    }
}

// gtheta[b][k] = the blocks' rows added in a fixed order, rounded to fp32 once.  One block of twelve waves per batch element: wave k owns
// entry k, its lane t adds rows t, t + 64, ... in that order, then the butterfly - the same order on every call (the finalize of
// pulpo_inverse_consistency).  (One thread per entry walking all rows took 195 us for 1024 rows: a chain of dependent-latency loads.)
__global__ __launch_bounds__(768) void affine_warp_bwd_finalize_kernel(const double* __restrict__ ws, float* __restrict__ gtheta, int nblk) {
    const int b = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* r = ws + (long)b * nblk * 12 + k;
    double s = 0.0;
    for (int j = lane; j < nblk; j += 64) s += r[(long)j * 12];
    s = pulpo::wave_sum_d(s);
    if (lane == 0) gtheta[b * 12 + k] = (float)s;
}

// out = the field on df's grid whose warp of an image equals warp(df, warp(affine_field(theta), image)) up to the second interpolation.
// Per axis: q = the clamped coordinate of sample_coord(v, df(v), Sg, Si) on the image grid; p = A(q) there; the displacement whose sample
// index is p's, out = p (Sg-1)/(Si-1) - v  (= (idx + 0.5)(Sg-1)/Si - v with idx = p Si/(Si-1) - 0.5; p - v on equal grids).
template <int VEC>
__global__ __launch_bounds__(256) void affine_compose_kernel(const float* __restrict__ theta, const float* __restrict__ df, float* __restrict__ out, int Dg,
                                                               int Hg, int Wg, int Di, int Hi, int Wi) {
    const int b = blockIdx.y;
    const Affine A = affine_load(theta + (long)b * 12, Di, Hi, Wi);
    const long V = (long)Dg * Hg * Wg, n = V / VEC;
    const float rz = Dg == 1 ? 0.f : (float)(Dg - 1) / (float)(Di - 1), ry = (float)(Hg - 1) / (float)(Hi - 1), rx = (float)(Wg - 1) / (float)(Wi - 1);
    const float* f = df + (long)b * 3 * V;
    float* o = out + (long)b * 3 * V;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int vi = (int)(e * VEC);
        const int x = vi % Wg, y = (vi / Wg) % Hg, z = vi / (Wg * Hg);
        float in[3][VEC], r[3][VEC];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if constexpr (VEC == 4) {
                const float4 t = *reinterpret_cast<const float4*>(f + a * V + vi);
                in[a][0] = t.x; in[a][1] = t.y; in[a][2] = t.z; in[a][3] = t.w;
            } else {
                in[a][0] = f[a * V + vi];
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const Corner cz = sample_coord((float)z, in[0][k], Dg, Di);
            const Corner cy = sample_coord((float)y, in[1][k], Hg, Hi);
            const Corner cx = sample_coord((float)(x + k), in[2][k], Wg, Wi);
            float p[3];
            affine_pos(A, (float)cz.i0 + cz.f, (float)cy.i0 + cy.f, (float)cx.i0 + cx.f, p);
            r[0][k] = Dg == 1 ? 0.f : __fmaf_rn(p[0], rz, -(float)z);
            r[1][k] = __fmaf_rn(p[1], ry, -(float)y);
            r[2][k] = __fmaf_rn(p[2], rx, -(float)(x + k));
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(o + a * V + vi) = make_float4(r[a][0], r[a][1], r[a][2], r[a][3]);
            else o[a * V + vi] = r[a][0];
        }
    }
}

using pulpo::eblocks;

inline bool rows4(int W, const void* a, const void* b) { return W % 4 == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

inline int bwd_blocks(int Dg, int Hg, int Wg) { return pulpo_loss_blocks((int64_t)Dg * Hg * Wg); }

}  // namespace

PULPO_API int pulpo_affine_field(const float* theta, float* out, int B, int D, int H, int W, void* stream) {
    PULPO_REQUIRE(theta && out, "affine_field: null pointer");
    PULPO_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long)D * H * W < (1L << 31), "affine_field: B >= 1 and extents >= 1 (fewer than 2^31 voxels) expected");
    const long V = (long)D * H * W;
    hipStream_t st = (hipStream_t)stream;
    if (rows4(W, out, out))
        hipLaunchKernelGGL(affine_field_kernel<4>, dim3(eblocks(V / 4, 8192 / B + 1), B), dim3(256), 0, st, theta, out, D, H, W);
    else
        hipLaunchKernelGGL(affine_field_kernel<1>, dim3(eblocks(V, 8192 / B + 1), B), dim3(256), 0, st, theta, out, D, H, W);
    return pulpo::check_launch("affine_field");
}

PULPO_API int pulpo_affine_warp_fwd(const float* theta, const float* img, float* out, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi,
                                    void* stream) {
    PULPO_REQUIRE(theta && img && out, "affine_warp_fwd: null pointer");
    PULPO_REQUIRE(B >= 1 && B <= 65535 && C >= 1, "affine_warp_fwd: B >= 1 and C >= 1 expected");
    PULPO_REQUIRE(Dg >= 1 && Hg >= 1 && Wg >= 1 && Di >= 1 && Hi >= 1 && Wi >= 1 && (Dg > 1 || Di == 1),
                  "affine_warp_fwd: extents >= 1 expected (depth 1 = 2-D form, with a depth-1 image)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "affine_warp_fwd: grids of 2^31 voxels and more are not supported");
    const int nblk = pulpo::cdiv((long)Dg * Hg * Wg, 256);                     // (fewer than 2^23 blocks: one voxel per thread)
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL(affine_warp_fwd_kernel<1>, dim3(nblk, B), dim3(256), 0, st, theta, img, out, Dg, Hg, Wg, Di, Hi, Wi, C);
    else if (C == 3) hipLaunchKernelGGL(affine_warp_fwd_kernel<3>, dim3(nblk, B), dim3(256), 0, st, theta, img, out, Dg, Hg, Wg, Di, Hi, Wi, C);
    else hipLaunchKernelGGL(affine_warp_fwd_kernel<0>, dim3(nblk, B), dim3(256), 0, st, theta, img, out, Dg, Hg, Wg, Di, Hi, Wi, C);
    return pulpo::check_launch("affine_warp_fwd");
}

PULPO_API size_t pulpo_affine_warp_bwd_ws_bytes(int B, int Dg, int Hg, int Wg) {
    if (B <= 0 || Dg < 1 || Hg < 1 || Wg < 1) return 0;
    return (size_t)B * bwd_blocks(Dg, Hg, Wg) * 12 * sizeof(double);
}

PULPO_API int pulpo_affine_warp_bwd(const float* theta, const float* img, const float* gout, float* gtheta, void* ws, int B, int C, int Dg, int Hg,
                                    int Wg, int Di, int Hi, int Wi, void* stream) {
    PULPO_REQUIRE(theta && img && gout && gtheta, "affine_warp_bwd: null pointer");
    PULPO_REQUIRE(ws != nullptr, "affine_warp_bwd: workspace of pulpo_affine_warp_bwd_ws_bytes() bytes required");
    PULPO_REQUIRE(B >= 1 && B <= 65535 && C >= 1, "affine_warp_bwd: B >= 1 and C >= 1 expected");
    PULPO_REQUIRE(Dg >= 1 && Hg >= 1 && Wg >= 1 && Di >= 1 && Hi >= 1 && Wi >= 1 && (Dg > 1 || Di == 1),
                  "affine_warp_bwd: extents >= 1 expected (depth 1 = 2-D form, with a depth-1 image)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "affine_warp_bwd: grids of 2^31 voxels and more are not supported");
    const int nblk = bwd_blocks(Dg, Hg, Wg);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(affine_warp_bwd_kernel, dim3(nblk, B), dim3(256), 0, st, theta, img, gout, (double*)ws, Dg, Hg, Wg, Di, Hi, Wi, C);
    int rc = pulpo::check_launch("affine_warp_bwd");
    if (rc) return rc;
    hipLaunchKernelGGL(affine_warp_bwd_finalize_kernel, dim3(B), dim3(768), 0, st, (const double*)ws, gtheta, nblk);
    return pulpo::check_launch("affine_warp_bwd finalize");
}

PULPO_API int pulpo_affine_compose(const float* theta, const float* df, float* out, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream) {
    PULPO_REQUIRE(theta && df && out, "affine_compose: null pointer");
    PULPO_REQUIRE(B >= 1 && B <= 65535, "affine_compose: B >= 1 expected");
    PULPO_REQUIRE(Dg >= 1 && Hg > 1 && Wg > 1 && Di >= 1 && Hi > 1 && Wi > 1 && (Dg > 1) == (Di > 1),
                  "affine_compose: H, W > 1 on both grids expected (depth 1 = 2-D form, on both grids)");
    PULPO_REQUIRE((long)Dg * Hg * Wg < (1L << 31), "affine_compose: grids of 2^31 voxels and more are not supported");
    const long V = (long)Dg * Hg * Wg;
    hipStream_t st = (hipStream_t)stream;
    if (rows4(Wg, df, out))
        hipLaunchKernelGGL(affine_compose_kernel<4>, dim3(eblocks(V / 4, 8192 / B + 1), B), dim3(256), 0, st, theta, df, out, Dg, Hg, Wg, Di, Hi, Wi);
    else
        hipLaunchKernelGGL(affine_compose_kernel<1>, dim3(eblocks(V, 8192 / B + 1), B), dim3(256), 0, st, theta, df, out, Dg, Hg, Wg, Di, Hi, Wi);
    return pulpo::check_launch("affine_compose");
}
