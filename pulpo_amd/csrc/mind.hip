// MIND-SSC similarity term (modality-independent neighbourhood descriptor, self-similarity context).  No counterpart
// in the reference, whose losses all assume one contrast.  The per-voxel arithmetic and the index rules are in mind_core.h.
//
// Tile kernels (descriptor / cost / G): a workgroup stages the image tile(s) with a halo of d + 1 voxels in LDS - clamped into the volume,
// so every read after the staging is a plain LDS read - and each thread forms the twelve patch distances of its voxels from 27 x 6 LDS
// reads per image.  No descriptor goes to HBM in the cost and G kernels.
// Backward: pass 1 writes G_k = d cost / d D_k[pred] (times the mask weight) to the 12N scratch, pass 2 gathers the image gradient
// from it (mind::grad_gather).  Every reduction is per-workgroup partial -> pulpo_colsum / pulpo_masked_finish in double, and the
// gradient is a gather: no atomics, bit-identical run to run.
#include "common.h"
#include "mind_core.h"

namespace {

constexpr int kLdsBytes = 65536 - 64;      // (the reduction's few static words share the 64 KiB)
constexpr int kMaxGrid = 2048;

struct Tiling {
    int lz, ly, lx;           // log2 of the output tile's extents
    int nz, ny, nx;           // tiles per axis
    long ntile;               // over the batch as well
    int elems;                // floats of one staged image tile
};

// the largest tile, from 8 x 8 x 32 down, whose nimg staged images fit in 64 KiB of LDS; false: the dilation is too large for any
static bool pick_tiling(int B, int D, int H, int W, int d, int nimg, Tiling& t) {
    const int h = d + 1;
    t.lz = 3, t.ly = 3, t.lx = W <= 8 ? 3 : W <= 16 ? 4 : 5;
    for (;;) {
        const long e = (long)((1 << t.lz) + 2 * h) * ((1 << t.ly) + 2 * h) * ((1 << t.lx) + 2 * h);
        if (e * nimg * (long)sizeof(float) <= kLdsBytes) {
            t.elems = (int)e;
            break;
        }
        if (t.lz >= t.ly && t.lz > 1) --t.lz;
        else if (t.ly > 1) --t.ly;
        else if (t.lx > 3) --t.lx;
        else if (t.lz > 0) --t.lz;
        else if (t.ly > 0) --t.ly;
        else return false;
    }
    t.nz = pulpo::cdiv(D, 1 << t.lz), t.ny = pulpo::cdiv(H, 1 << t.ly), t.nx = pulpo::cdiv(W, 1 << t.lx);
    t.ntile = (long)B * t.nz * t.ny * t.nx;
    return true;
}

using pulpo::block_sum_256;

// MODE 0: out[k N + e] = f_k of img0                                            (one image staged)
// MODE 1: partial[block] = sum of cost; with masks partial[2 block] = sum of m cost, partial[2 block + 1] = sum of m
// MODE 2: out[k N + e] = m * d cost / d D_k[img1]
// img0 = y_true, img1 = y_pred.  Workgroups walk the tiles in a strided loop; a tile's voxels are dealt to the 256 threads x-fastest.
template <int MODE>
__global__ __launch_bounds__(256) void mind_tile_kernel(const float* __restrict__ img0, const float* __restrict__ img1, const float* __restrict__ wa,
                                                          const float* __restrict__ wb, float* __restrict__ out, float* __restrict__ partial, long N,
                                                          int D, int H, int W, int d, float eps, Tiling tl) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float sh[4];
    const int h = d + 1;
    const int TZ = 1 << tl.lz, TY = 1 << tl.ly, TX = 1 << tl.lx;
    const int ey = TY + 2 * h, ex = TX + 2 * h;
    constexpr int NI = MODE == 0 ? 1 : 2;                // staged images, interleaved per voxel
    const long V = (long)D * H * W;
    [[maybe_unused]] float local = 0.f, msum = 0.f;
    for (long tile = blockIdx.x; tile < tl.ntile; tile += gridDim.x) {
        const int tx = (int)(tile % tl.nx), ty = (int)((tile / tl.nx) % tl.ny), tz = (int)((tile / ((long)tl.nx * tl.ny)) % tl.nz);
        const long b = tile / ((long)tl.nx * tl.ny * tl.nz);
        const int oz = tz * TZ - h, oy = ty * TY - h, ox = tx * TX - h;
        const float* p0 = img0 + b * V;
        [[maybe_unused]] const float* p1 = MODE != 0 ? img1 + b * V : nullptr;
        __syncthreads();                                   // the previous tile's reads are done
        for (int i = threadIdx.x; i < tl.elems; i += 256) {
            const int jx = i % ex, jy = (i / ex) % ey, jz = i / (ex * ey);
            const long g = ((long)mind::clampi(oz + jz, D - 1) * H + mind::clampi(oy + jy, H - 1)) * W + mind::clampi(ox + jx, W - 1);
            if constexpr (MODE == 0) lds[i] = p0[g];
            else *reinterpret_cast<float2*>(lds + 2 * i) = make_float2(p0[g], p1[g]);
        }
        __syncthreads();
        for (int v = threadIdx.x; v < TZ * TY * TX; v += 256) {
            const int x = tx * TX + (v & (TX - 1)), y = ty * TY + ((v >> tl.lx) & (TY - 1)), z = tz * TZ + (v >> (tl.lx + tl.ly));
            if (x >= W || y >= H || z >= D) continue;
            const long e = b * V + ((long)z * H + y) * W + x;
            float Dk[NI][mind::NCH], f0[mind::NCH], mk[mind::NCH], Vv;
            mind::patch_dist<NI>(lds, oz, oy, ox, ey, ex, D, H, W, d, z, y, x, Dk);
            mind::descriptor(Dk[0], eps, f0, mk, Vv);
            if constexpr (MODE == 0) {
#pragma unroll
                for (int k = 0; k < mind::NCH; ++k) out[k * N + e] = f0[k];
            } else {
                float f1[mind::NCH];
                const int am = mind::descriptor(Dk[NI - 1], eps, f1, mk, Vv);
                const float m = wa == nullptr ? 1.f : (wb != nullptr ? wa[e] * wb[e] : wa[e]);
                if constexpr (MODE == 1) {
                    local += m * mind::cost(f1, f0);
                    msum += m;
                } else {
                    float G[mind::NCH];
                    mind::cost_grad(f1, f0, mk, Vv, am, G);
#pragma unroll
                    for (int k = 0; k < mind::NCH; ++k) out[k * N + e] = m * G[k];
                }
            }
        }
    }
    if constexpr (MODE == 1) {
        const float t = block_sum_256(local, sh);
        if (wa != nullptr) {
            const float tm = block_sum_256(msum, sh);
            if (threadIdx.x == 0) {
                partial[2 * blockIdx.x] = t;
                partial[2 * blockIdx.x + 1] = tm;
            }
        } else if (threadIdx.x == 0) partial[blockIdx.x] = t;
    }
}

// pass 2 of the backward: gpred = coef * gscale * gather of G (mind::grad_gather), one voxel per thread in a strided loop
__global__ __launch_bounds__(256) void mind_gather_kernel(const float* __restrict__ G, const float* __restrict__ pred, const float* __restrict__ gscale,
                                                            float coef, float* __restrict__ gpred, long N, int D, int H, int W, int d) {
    const float k0 = coef * (gscale != nullptr ? gscale[0] : 1.f);
    const long V = (long)D * H * W;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const long b = e / V;
        const int v = (int)(e - b * V);
        const int x = v % W, y = (v / W) % H, z = v / (W * H);
        gpred[e] = k0 * mind::grad_gather(G + b * V, N, pred + b * V, D, H, W, d, z, y, x);
    }
}

static int check_shape(const char* who, int B, int D, int H, int W, int d, float eps) {
    PULPO_REQUIRE(B > 0 && D >= 2 && H >= 2 && W >= 2, "%s: every extent must be >= 2 (got B %d, %d x %d x %d)", who, B, D, H, W);
    PULPO_REQUIRE((long)D * H * W < (1L << 31), "%s: a volume has at most 2^31 - 1 voxels", who);
    PULPO_REQUIRE(d >= 1, "%s: dilation must be >= 1 (got %d)", who, d);
    PULPO_REQUIRE(eps > 0.f, "%s: eps must be > 0", who);
    return 0;
}

template <int MODE>
static int launch_tiles(const char* who, const float* img0, const float* img1, const float* wa, const float* wb, float* out, float* partial, int B, int D,
                        int H, int W, int d, float eps, hipStream_t st) {
    Tiling tl;
    PULPO_REQUIRE(pick_tiling(B, D, H, W, d, MODE == 0 ? 1 : 2, tl), "%s: dilation %d is too large for the 64 KiB LDS tile", who, d);
    const int grid = (int)std::min<long>(tl.ntile, kMaxGrid);
    const size_t lds = (size_t)tl.elems * (MODE == 0 ? 1 : 2) * sizeof(float);
    hipLaunchKernelGGL(mind_tile_kernel<MODE>, dim3(grid), dim3(256), lds, st, img0, img1, wa, wb, out, partial, (long)B * D * H * W, D, H, W, d, eps, tl);
    return pulpo::check_launch(who);
}

}  // namespace

// rows of the cost partials of pulpo_mind_fwd (one per workgroup); 0 for arguments the entry points refuse
PULPO_API int pulpo_mind_blocks(int B, int D, int H, int W, int d) {
    Tiling tl;
    if (B <= 0 || D < 2 || H < 2 || W < 2 || d < 1 || !pick_tiling(B, D, H, W, d, 2, tl)) return 0;
    return (int)std::min<long>(tl.ntile, kMaxGrid);
}

PULPO_API int pulpo_mind_descriptor(const float* I, float* out, int B, int D, int H, int W, int d, float eps, void* stream) {
    PULPO_REQUIRE(I && out, "mind_descriptor: bad arguments");
    if (int rc = check_shape("mind_descriptor", B, D, H, W, d, eps)) return rc;
    return launch_tiles<0>("mind_descriptor", I, nullptr, nullptr, nullptr, out, nullptr, B, D, H, W, d, eps, (hipStream_t)stream);
}

PULPO_API int pulpo_mind_fwd(const float* y_true, const float* y_pred, const float* wa, const float* wb, float* partial, int B, int D, int H, int W, int d,
                             float eps, void* stream) {
    PULPO_REQUIRE(y_true && y_pred && partial && (wa || !wb), "mind_fwd: bad arguments");
    if (int rc = check_shape("mind_fwd", B, D, H, W, d, eps)) return rc;
    return launch_tiles<1>("mind_fwd", y_true, y_pred, wa, wb, nullptr, partial, B, D, H, W, d, eps, (hipStream_t)stream);
}

PULPO_API int pulpo_mind_bwd(const float* y_true, const float* y_pred, const float* wa, const float* wb, float* scratch, const float* gscale, float coef,
                             float* gpred, int B, int D, int H, int W, int d, float eps, void* stream) {
    PULPO_REQUIRE(y_true && y_pred && scratch && gpred && (wa || !wb), "mind_bwd: bad arguments");
    if (int rc = check_shape("mind_bwd", B, D, H, W, d, eps)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_tiles<2>("mind_bwd G", y_true, y_pred, wa, wb, scratch, nullptr, B, D, H, W, d, eps, st)) return rc;
    const long N = (long)B * D * H * W;
    const int grid = (int)std::max<long>(1, std::min<long>((N + 255) / 256, 8192));
    hipLaunchKernelGGL(mind_gather_kernel, dim3(grid), dim3(256), 0, st, scratch, y_pred, gscale, coef, gpred, N, D, H, W, d);
    return pulpo::check_launch("mind_bwd gather");
}
