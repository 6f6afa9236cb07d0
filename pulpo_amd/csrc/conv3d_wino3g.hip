// Winograd F(2x2x2, 3x3x3) as 64 batched GEMMs, for the coarse pyramid levels (20^3, 10^3) whose extents are not whole 4 x 8 x 8 tiles.
// conv3d_wino3.hip keeps the transformed operand in LDS and so needs whole tiles and enough of them; a 20^3 volume has 45 ragged tiles, which
// leaves the (y, x) kernel with split-K slabs bound by its parallelism.  In the transformed domain the same level is
// 1000 output blocks x 64 points: three plain kernels, no atomics, every sum in a fixed order.
//   1. wino3g_input_kernel       V[p][row][k] = (B^T x B^T x B^T) d   row = 2x2x2 output block (b, z/2, y/2, x/2), d its 4x4x4 patch, zeros outside
//                                the volume; rows padded with zeros to the GEMM's 128-row tile
//   2. conv3d_k3_wino3_gemm      M[p] = V[p] . U[p], p = 0..63, on v_mfma_f32_32x32x2_f32; U is conv3d_wino3.hip's weight pack, read as it is
//                                (wino3_pack.h: [chunk][point][NPad][8]), so PulpoPackJob kind 4 refreshes it
//   3. wino3g_output_kernel      out = (A^T x A^T x A^T) M + bias through the result's strides, with the BatchNorm partial rows
//                                (pulpo_conv3d_k3_stat_tiles() rows, every row written: row r sums the blocks [nblk r / nrow, nblk (r + 1) / nrow) -
//                                any partition serves the double-precision finalize, as for splitk_reduce_kernel) or the eval-mode store
// B^T = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], A^T = [[1, 1, 1, 0], [0, 1, -1, -1]]: conv3d_wino3.hip's coefficients.
#include "conv_shared.h"
#include "head_bn.h"

PULPO_API int pulpo_conv3d_k3_stat_tiles(int B, int D, int H, int W);
PULPO_API int pulpo_conv3d_k3_algo(int B, int D, int H, int W, int K, int N);

namespace {

using namespace pulpo_conv;

constexpr int G_BM = 128;                        // rows of a GEMM block tile: four waves x 32 rows
constexpr int G_BK = 32;                         // reduction channels per step: four 8-channel chunks of the weight pack
constexpr int G_LS = G_BK + 4;                   // LDS row pitch in floats: 36 = 4 mod 32, the 16 lanes of a ds_read_b128 group fall into 16 different slots

__device__ __forceinline__ void wino3g_bt(float d0, float d1, float d2, float d3, float& t0, float& t1, float& t2, float& t3) {
    t0 = d0 - d2; t1 = d1 + d2; t2 = d2 - d1; t3 = d1 - d3;
}

// one thread per (row, reduction channel): e = row * K + k, consecutive lanes read and write consecutive channels
__global__ __launch_bounds__(256) void wino3g_input_kernel(const float* __restrict__ in, long in_bs, long in_ps, long in_cs, float* __restrict__ V, int D,
                                                           int H, int W, int K, long nrows, long rows_pad) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    const long plane = rows_pad * K;
    if (e >= plane) return;
    const long row = e / K;
    const int k = (int)(e - row * K);
    float d[4][4][4];
    const int W2 = W >> 1, H2 = H >> 1, D2 = D >> 1;
    const bool live = row < nrows;
    long q = live ? row : 0;
    const int bx = (int)(q % W2); q /= W2;
    const int by = (int)(q % H2); q /= H2;
    const int bz = (int)(q % D2);
    const long b = q / D2;
    const float* src = in + b * in_bs + (long)k * in_cs;
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const int iz = 2 * bz - 1 + z;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int iy = 2 * by - 1 + y;
            const bool rowok = live && (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int ix = 2 * bx - 1 + x;
                d[z][y][x] = (rowok && (unsigned)ix < (unsigned)W) ? src[((long)(iz * H + iy) * W + ix) * in_ps] : 0.f;
            }
        }
    }
#pragma unroll
    for (int z = 0; z < 4; ++z)
#pragma unroll
        for (int y = 0; y < 4; ++y) wino3g_bt(d[z][y][0], d[z][y][1], d[z][y][2], d[z][y][3], d[z][y][0], d[z][y][1], d[z][y][2], d[z][y][3]);
#pragma unroll
    for (int z = 0; z < 4; ++z)
#pragma unroll
        for (int x = 0; x < 4; ++x) wino3g_bt(d[z][0][x], d[z][1][x], d[z][2][x], d[z][3][x], d[z][0][x], d[z][1][x], d[z][2][x], d[z][3][x]);
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) wino3g_bt(d[0][y][x], d[1][y][x], d[2][y][x], d[3][y][x], d[0][y][x], d[1][y][x], d[2][y][x], d[3][y][x]);
#pragma unroll
    for (int z = 0; z < 4; ++z)
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int x = 0; x < 4; ++x) V[(long)(z * 16 + y * 4 + x) * plane + e] = d[z][y][x];
}

}  // namespace

// M[p][row][n] = sum_k V[p][row][k] * U[chunk k / 8][p][n][k % 8].  Block tile 128 x (32 RN) x 32, four waves, wave w = rows 32 w .. 32 w + 31 against
// all RN column tiles.  One LDS image, the next step's operands wait in registers while this step multiplies; several workgroups per CU cover
// the two barriers of a step.  Lane (i = lane & 31, kk = lane >> 5) feeds MFMA j of a chunk with k = 4 kk + j for BOTH operands: one float4 each.
// (Outside the anonymous namespace: the kernel's name is what a trace shows, and the step's FLOP accounting looks for "wino3" in it.)
// Four waves per SIMD = four workgroups per CU: 64 x 8 row tiles x 2 column tiles of a 192 -> 192 layer at 20^3 are 1024 workgroups, one
// resident round of 256 CUs (the compiler's own choice, 144 registers, leaves a quarter of them to a second round); no spills at 128.
template <int RN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv3d_k3_wino3_gemm(const float* __restrict__ V, const float* __restrict__ U, float* __restrict__ M, long rows_pad,
                                                            int K, int N, int NPad, int nrt, int nct) {
    constexpr int BN = RN * 32;
    __shared__ __attribute__((aligned(16))) float As[G_BM * G_LS];
    __shared__ __attribute__((aligned(16))) float Bs[BN * G_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, kk = lane >> 5;
    const int bid = pulpo::xcd_remap(blockIdx.x, gridDim.x);
    const int ct = bid % nct;
    const int rt = (bid / nct) % nrt;
    const int p = bid / (nct * nrt);
    const float* Vp = V + ((long)p * rows_pad + (long)rt * G_BM) * K;
    const float* Up = U + ((long)p * NPad + ct * BN) * 8;
    const long chunk_stride = 64L * NPad * 8;
    const int nchunk = K >> 3;
    const int nstep = (nchunk + 3) >> 2;

    float4 pa[4], pb[RN];
    auto fetch = [&](int s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = tid + 256 * j;
            const int q = idx & 7, r = idx >> 3;
            const int k = s * G_BK + 4 * q;
            pa[j] = k < K ? *reinterpret_cast<const float4*>(Vp + (long)r * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int idx = tid + 256 * j;
            const int h = idx & 1, n = (idx >> 1) % BN, cc = idx / (2 * BN);
            const int chunk = s * 4 + cc;
            pb[j] = (chunk < nchunk && ct * BN + n < NPad) ? *reinterpret_cast<const float4*>(Up + chunk * chunk_stride + n * 8 + 4 * h)
                                                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = tid + 256 * j;
            *reinterpret_cast<float4*>(As + (idx >> 3) * G_LS + 4 * (idx & 7)) = pa[j];
        }
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int idx = tid + 256 * j;
            const int h = idx & 1, n = (idx >> 1) % BN, cc = idx / (2 * BN);
            *reinterpret_cast<float4*>(Bs + n * G_LS + cc * 8 + 4 * h) = pb[j];
        }
    };

    f32x16 acc[RN];
#pragma unroll
    for (int t = 0; t < RN; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    fetch(0);
    for (int s = 0; s < nstep; ++s) {
        stage();
        __syncthreads();
        if (s + 1 < nstep) fetch(s + 1);
        const float* ar = As + (wave * 32 + i) * G_LS + 4 * kk;
        const float* br = Bs + i * G_LS + 4 * kk;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a4 = *reinterpret_cast<const float4*>(ar + g * 8);
            float4 b4[RN];
#pragma unroll
            for (int t = 0; t < RN; ++t) b4[t] = *reinterpret_cast<const float4*>(br + t * 32 * G_LS + g * 8);
#pragma unroll
            for (int t = 0; t < RN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < RN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < RN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < RN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4[t].w, acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // accumulator register r of lane (i, kk) = row (r & 3) + 8 (r >> 2) + 4 kk of the wave's 32, column i
    float* Mp = M + ((long)p * rows_pad + (long)rt * G_BM + wave * 32) * N;
#pragma unroll
    for (int t = 0; t < RN; ++t) {
        const int n = ct * BN + t * 32 + i;
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Mp[(long)((r & 3) + 8 * (r >> 2) + 4 * kk) * N + n] = acc[t][r];
        }
    }
}

namespace {

// grid (statistics rows, groups of 32 output channels), 256 threads = 32 channels x 8 block lanes
__global__ __launch_bounds__(256) void wino3g_output_kernel(const float* __restrict__ M, const float* __restrict__ bias, const float* __restrict__ coef,
                                                            float slope, float* __restrict__ out, long out_bs, long out_ps, long out_cs,
                                                            float* __restrict__ stats, int D, int H, int W, int N, long nblk, long rows_pad, int nrow) {
    __shared__ float red[2][256];
    const int r = blockIdx.x, c = blockIdx.y * 32 + (threadIdx.x & 31), bl = threadIdx.x >> 5;
    const long b0 = nblk * r / nrow, b1 = nblk * (r + 1) / nrow;
    const bool cok = c < N;
    const float bv = (cok && bias != nullptr) ? bias[c] : 0.f;
    const bool fuse = cok && coef != nullptr;
    const float fsc = fuse ? coef[2 * N + c] : 1.f, fsh = fuse ? coef[3 * N + c] : 0.f;
    const int W2 = W >> 1, H2 = H >> 1, D2 = D >> 1;
    const long plane = rows_pad * N;
    float s = 0.f, sq = 0.f;
    if (cok)
        for (long blk = b0 + bl; blk < b1; blk += 8) {
            const float* m = M + blk * N + c;
            float tz[4][2][2];                      // [pz][oy][ox]
#pragma unroll
            for (int pz = 0; pz < 4; ++pz) {
                float ty[4][2];                     // [py][ox]
#pragma unroll
                for (int py = 0; py < 4; ++py) {
                    const float* mp = m + (long)(pz * 16 + py * 4) * plane;
                    const float m0 = mp[0], m1 = mp[plane], m2 = mp[2 * plane], m3 = mp[3 * plane];
                    ty[py][0] = m0 + m1 + m2;
                    ty[py][1] = m1 - m2 - m3;
                }
#pragma unroll
                for (int ox = 0; ox < 2; ++ox) {
                    tz[pz][0][ox] = ty[0][ox] + ty[1][ox] + ty[2][ox];
                    tz[pz][1][ox] = ty[1][ox] - ty[2][ox] - ty[3][ox];
                }
            }
            long q = blk;
            const int bx = (int)(q % W2); q /= W2;
            const int by = (int)(q % H2); q /= H2;
            const int bz = (int)(q % D2);
            const long b = q / D2;
            float* o = out + b * out_bs + (long)c * out_cs;
#pragma unroll
            for (int oy = 0; oy < 2; ++oy)
#pragma unroll
                for (int ox = 0; ox < 2; ++ox) {
                    float v[2];
                    v[0] = tz[0][oy][ox] + tz[1][oy][ox] + tz[2][oy][ox] + bv;
                    v[1] = tz[1][oy][ox] - tz[2][oy][ox] - tz[3][oy][ox] + bv;
#pragma unroll
                    for (int oz = 0; oz < 2; ++oz) {
                        s += v[oz];
                        sq += v[oz] * v[oz];
                        const float w = fuse ? pulpo::bn_lrelu(v[oz], fsc, fsh, slope) : v[oz];
                        o[((long)((2 * bz + oz) * H + 2 * by + oy) * W + 2 * bx + ox) * out_ps] = w;
                    }
                }
        }
    if (stats != nullptr) {
        red[0][threadIdx.x] = s;
        red[1][threadIdx.x] = sq;
        __syncthreads();
        if (threadIdx.x < 64) {
            const int which = threadIdx.x >> 5, cc = threadIdx.x & 31;
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += red[which][k * 32 + cc];
            if (blockIdx.y * 32 + cc < N) stats[((long)r * 2 + which) * N + blockIdx.y * 32 + cc] = t;
        }
    }
}

long wino3g_blocks(int B, int D, int H, int W) { return (long)B * (D / 2) * (H / 2) * (W / 2); }
long wino3g_rows_pad(int B, int D, int H, int W) { return (wino3g_blocks(B, D, H, W) + G_BM - 1) / G_BM * G_BM; }

// shapes the entry point takes (any size): even extents, 8-channel chunks of the weight pack, whole float4s of output channels
bool wino3g_entry_ok(int B, int D, int H, int W, int K, int N) {
    return B > 0 && D > 0 && H > 0 && W > 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && K > 0 && K % 8 == 0 && N > 0 && N % 4 == 0;
}

}  // namespace

// 1 where the forward / data-gradient convolution of a shape runs here by default (fp32 operands): the layers from 128 channels up of volumes
// with 125 .. 1000 output blocks that the (y, x) kernel runs today (pulpo_conv3d_k3_algo() == 2: not whole 4 x 8 x 8 tiles, or too few of them for
// conv3d_wino3.hip) - 128 -> 192, 192 -> 192, 288 -> 192 at 20^3 and 192 -> 192 at 10^3 of the 160^3 pyramid.  pulpo_conv3d_k3_algo() keeps that
// answer: it names the kernel behind pulpo_conv3d_k3_fwd_wino2, which still takes these shapes.
PULPO_API int pulpo_conv3d_k3_wino3g_ok(int B, int D, int H, int W, int K, int N) {
    if (!wino3g_entry_ok(B, D, H, W, K, N) || N % 32 != 0 || pulpo_conv3d_k3_algo(B, D, H, W, K, N) != 2) return 0;
    const long blocks = wino3g_blocks(B, D, H, W);
    return blocks >= 125 && blocks <= 1000 && std::min(K, N) >= 128;
}

PULPO_API size_t pulpo_conv3d_k3_fwd_wino3g_scratch_floats(int B, int D, int H, int W, int K, int N) {
    if (!wino3g_entry_ok(B, D, H, W, K, N)) return 0;
    return (size_t)64 * wino3g_rows_pad(B, D, H, W) * ((size_t)K + N);
}

PULPO_API int pulpo_conv3d_k3_fwd_wino3g(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias,
                                         const float* coef, float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats,
                                         float* scratch, int B, int D, int H, int W, int K, int N, void* stream) {
    PULPO_REQUIRE(in && wp && out && scratch, "conv3d_k3_fwd_wino3g: null pointer");
    PULPO_REQUIRE(wino3g_entry_ok(B, D, H, W, K, N),
                  "conv3d_k3_fwd_wino3g: shape %dx%dx%d, %d -> %d channels: even extents, K %% 8 == 0 and N %% 4 == 0 required", D, H, W, K, N);
    PULPO_REQUIRE(!(coef && stats), "conv3d_k3_fwd_wino3g: batch statistics are not available from the fused eval-mode epilogue");
    PULPO_REQUIRE((((uintptr_t)wp | (uintptr_t)scratch) & 15) == 0, "conv3d_k3_fwd_wino3g: packed weights and scratch must be 16-byte aligned");
    const long nblk = wino3g_blocks(B, D, H, W), rows_pad = wino3g_rows_pad(B, D, H, W);
    const int rn = N % 96 == 0 ? 3 : 2;
    const int nrt = (int)(rows_pad / G_BM), nct = pulpo::cdiv(N, rn * 32);
    PULPO_REQUIRE(64L * nrt * nct < (1L << 31) && rows_pad * K < (1L << 31) * 256, "conv3d_k3_fwd_wino3g: grid too large");
    PULPO_REQUIRE(nct * rn * 32 <= npad(N), "conv3d_k3_fwd_wino3g: column tiles exceed the weight pack");
    hipStream_t st = (hipStream_t)stream;
    float* V = scratch;
    float* M = scratch + 64 * rows_pad * K;
    hipLaunchKernelGGL(wino3g_input_kernel, dim3(pulpo::cdiv(rows_pad * K, 256)), dim3(256), 0, st, in, (long)in_bs, (long)in_ps, (long)in_cs, V, D, H, W, K,
                       nblk, rows_pad);
    int rc = pulpo::check_launch("wino3g_input");
    if (rc != 0) return rc;
    if (rn == 3) hipLaunchKernelGGL((conv3d_k3_wino3_gemm<3>), dim3(64 * nrt * nct), dim3(256), 0, st, V, wp, M, rows_pad, K, N, npad(N), nrt, nct);
    else hipLaunchKernelGGL((conv3d_k3_wino3_gemm<2>), dim3(64 * nrt * nct), dim3(256), 0, st, V, wp, M, rows_pad, K, N, npad(N), nrt, nct);
    rc = pulpo::check_launch("conv3d_k3_wino3_gemm");
    if (rc != 0) return rc;
    const int nrow = pulpo_conv3d_k3_stat_tiles(B, D, H, W);
    hipLaunchKernelGGL(wino3g_output_kernel, dim3(nrow, pulpo::cdiv(N, 32)), dim3(256), 0, st, M, bias, coef, slope, out, (long)out_bs, (long)out_ps,
                       (long)out_cs, stats, D, H, W, N, nblk, rows_pad, nrow);
    return pulpo::check_launch("wino3g_output");
}
