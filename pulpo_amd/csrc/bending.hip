// Bending-energy regulariser of a displacement field (no counterpart in the reference).
//
//   e(q) = u_xx^2 + u_yy^2 + u_zz^2 + 2 u_xy^2 + 2 u_xz^2 + 2 u_yz^2     central differences, at INTERIOR voxels q only (1 .. extent - 2)
//   loss = coef * sum over (planes, interior voxels) of e                  coef = lamb * D*H*W / (nplanes * n_interior)
//   grad = 2 coef * sum_k w_k A_k^T (M . A_k u)                            M the interior mask, w = (1, 1, 1, 2, 2, 2)
// A depth of 1 is the 2-D form: no z term.
//
// One launch each.  A workgroup of 256 owns a kTY x kTX column of one plane (one (batch, component) volume), zc planes deep, and marches along
// z with a ring of planes in LDS: 2 R + 1 planes are read per output plane (R = 1 for the value, 2 for the gradient), one more slot receives the
// next plane meanwhile, so the march has one barrier per plane.  A plane of the ring is the tile plus a halo, out-of-volume positions zero; it
// is fetched to registers one iteration ahead (16-byte loads where W % 4 == 0 and the field is 16-byte aligned, 4-byte loads otherwise) and
// written to LDS after the current plane's arithmetic.  Every tap is an LDS read; the six stencils are symmetric, so the gradient is a gather of
// the 25 taps (axis +-1, +-2; the in-plane diagonals (+-2, +-2) of the three coordinate planes; the centre) with M folded in as 0/1 factors of
// the nine neighbour positions - no atomics, no scratch, bit-identical from run to run.  Indices inside a plane are 32-bit, plane bases 64-bit.
#include "common.h"

namespace {

constexpr int kTX = 32, kTY = 16;                // tile of a workgroup (x, y)
// planes per march: the longest of kZC whose grid still has kMinBlocks workgroups, else the shortest.  A march pays the halo planes once
// (2 R of them) but is a chain of dependent plane fetches: the pyramid's small levels are latency bound and want many short marches
constexpr int kZC[3] = {16, 8, 4};
constexpr long kMinBlocks = 1024;
constexpr int kPad = 4;                          // LDS columns in front of the tile: the halo (<= 2) rounded up to one 16-byte group
constexpr int kPitch = kTX + 2 * kPad;           // 40 floats: rows stay 16-byte aligned; a wave's 32-lane halves read one row each, conflict-free
constexpr int kRows = 256 / kTX;                 // rows of the tile a pass of the 256 threads covers (8): kTY / kRows voxels per thread
static_assert(kTY % kRows == 0 && kTX % 4 == 0, "tile shape");

struct Tile {
    int x0, y0, zb, ze;                          // first voxel of the tile, planes [zb, ze) of the march
    long vol;                                    // element offset of the tile's volume (plane * D * H * W)
};

// logical block -> tile.  Neighbouring tiles (which share halos) get neighbouring logical ids on one XCD
__device__ __forceinline__ Tile tile_of_block(int D, int H, int W, int zc) {
    const int ntx = (W + kTX - 1) / kTX, nty = (H + kTY - 1) / kTY, nzc = (D + zc - 1) / zc;
    int b = pulpo::xcd_remap((int)blockIdx.x, (int)gridDim.x);
    Tile t;
    t.x0 = (b % ntx) * kTX;
    b /= ntx;
    t.y0 = (b % nty) * kTY;
    b /= nty;
    t.zb = (b % nzc) * zc;
    t.ze = min(t.zb + zc, D);
    t.vol = (long)(b / nzc) * D * H * W;
    return t;
}

// one plane of the ring on its way from global memory to LDS: rows y0 - R .. y0 + kTY + R - 1
template <int R, bool VEC>
struct Stage {
    static constexpr int kHR = kTY + 2 * R;                              // rows with halo
    static constexpr int kCols = VEC ? kPitch / 4 : kTX + 2 * R;         // items per row: 16-byte groups from x0 - 4, or floats from x0 - R
    static constexpr int kItems = kHR * kCols;
    static constexpr int kPer = (kItems + 255) / 256;
    static constexpr int kPlane = kHR * kPitch;                          // floats of one ring slot
    float4 v4;
    float v[VEC ? 1 : kPer];

    __device__ __forceinline__ void load(const float* __restrict__ vol, const Tile& t, int z, int D, int H, int W) {
        const bool zin = z >= 0 && z < D;
        const float* __restrict__ pl = vol + (long)(zin ? z : 0) * H * W;
        if constexpr (VEC) {
            v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const int i = threadIdx.x;
            if (i < kItems) {
                const int row = i / kCols, c = i - row * kCols;
                const int y = t.y0 - R + row, x = t.x0 - kPad + 4 * c;
                if (zin && y >= 0 && y < H && x >= 0 && x < W) v4 = *reinterpret_cast<const float4*>(pl + y * W + x);     // W % 4 == 0: all four in
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int i = threadIdx.x + 256 * k;
                const int row = i / kCols, c = i - row * kCols;
                const int y = t.y0 - R + row, x = t.x0 - R + c;
                v[k] = (i < kItems && zin && y >= 0 && y < H && x >= 0 && x < W) ? pl[y * W + x] : 0.f;
            }
        }
    }

    __device__ __forceinline__ void write(float* __restrict__ slot) const {
        if constexpr (VEC) {
            const int i = threadIdx.x;
            if (i < kItems) {
                const int row = i / kCols, c = i - row * kCols;
                *reinterpret_cast<float4*>(slot + row * kPitch + 4 * c) = v4;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int i = threadIdx.x + 256 * k;
                const int row = i / kCols, c = i - row * kCols;
                if (i < kItems) slot[row * kPitch + kPad - R + c] = v[k];
            }
        }
    }
};

__device__ __forceinline__ float inside(int i, int n) { return (i >= 1 && i <= n - 2) ? 1.f : 0.f; }

// ------------------------------------------------------------------------------------------------ value
template <bool VEC>
__global__ __launch_bounds__(256) void bending_fwd_kernel(const float* __restrict__ df, int D, int H, int W, int zc,
                                                          float* __restrict__ partial) {
    constexpr int R = 1, NS = 2 * R + 2;
    using S = Stage<R, VEC>;
    __shared__ __attribute__((aligned(16))) float ring[NS * S::kPlane];
    __shared__ float sh[4];
    const Tile t = tile_of_block(D, H, W, zc);
    const float* __restrict__ vol = df + t.vol;
    const bool flat = D == 1;
    const int lx = threadIdx.x % kTX, ly = threadIdx.x / kTX;
    const bool xin = t.x0 + lx >= 1 && t.x0 + lx <= W - 2;

    S st;
    {                                                        // planes zb - R .. zb + R into slots 0 .. 2 R: all loads in flight, then the writes
        S pro[2 * R + 1];
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) pro[j].load(vol, t, t.zb - R + j, D, H, W);
        st.load(vol, t, t.zb + R + 1, D, H, W);
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) pro[j].write(ring + j * S::kPlane);
    }
    __syncthreads();

    float local = 0.f;
    int base = 0;                                            // slot of plane z - R
    for (int z = t.zb; z < t.ze; ++z) {
        const float* __restrict__ pm = ring + (base % NS) * S::kPlane;
        const float* __restrict__ pc = ring + ((base + 1) % NS) * S::kPlane;
        const float* __restrict__ pp = ring + ((base + 2) % NS) * S::kPlane;
        const bool zin = flat || (z >= 1 && z <= D - 2);
        if (zin && xin) {
#pragma unroll
            for (int k = 0; k < kTY / kRows; ++k) {
                const int y = t.y0 + ly + kRows * k;
                if (y >= 1 && y <= H - 2) {
                    const int o = (ly + kRows * k + R) * kPitch + lx + kPad;
                    const float c = pc[o];
                    const float uxx = pc[o + 1] - 2.f * c + pc[o - 1];
                    const float uyy = pc[o + kPitch] - 2.f * c + pc[o - kPitch];
                    const float uxy = 0.25f * (pc[o + kPitch + 1] - pc[o + kPitch - 1] - pc[o - kPitch + 1] + pc[o - kPitch - 1]);
                    float e = uxx * uxx + uyy * uyy + 2.f * uxy * uxy;
                    if (!flat) {
                        const float uzz = pp[o] - 2.f * c + pm[o];
                        const float uxz = 0.25f * (pp[o + 1] - pp[o - 1] - pm[o + 1] + pm[o - 1]);
                        const float uyz = 0.25f * (pp[o + kPitch] - pp[o - kPitch] - pm[o + kPitch] + pm[o - kPitch]);
                        e += uzz * uzz + 2.f * uxz * uxz + 2.f * uyz * uyz;
                    }
                    local += e;
                }
            }
        }
        if (z + 1 < t.ze) {
            st.write(ring + ((base + 2 * R + 1) % NS) * S::kPlane);      // plane z + R + 1 over plane z - R - 1 (last read one barrier ago)
            if (z + 2 < t.ze) st.load(vol, t, z + R + 2, D, H, W);
        }
        base = (base + 1) % NS;
        __syncthreads();
    }
    const float s = pulpo::block_sum_256(local, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------ gradient
// A^T (M . A u) at a voxel for a second difference along one axis: a .. e are u at offsets -2 .. 2, mm / mc / mp the mask at -1 / 0 / +1
__device__ __forceinline__ float axis_term(float a, float b, float c, float d, float e, float mm, float mc, float mp) {
    return mm * (a - 2.f * b + c) - 2.f * mc * (b - 2.f * c + d) + mp * (c - 2.f * d + e);
}

// 2 A^T (M . A u) at a voxel for the mixed difference of coordinates (a, b): u at offsets {-2, 0, 2}^2 (first index a), the masks of a and b at
// -1 / +1 (the third coordinate's mask is the caller's factor).  2 * (1/4) * (1/4) = 1/8
__device__ __forceinline__ float cross_term(float umm, float um0, float ump, float u0m, float u00, float u0p, float upm, float up0, float upp,
                                            float mam, float map, float mbm, float mbp) {
    return 0.125f * (map * mbp * (upp - up0 - u0p + u00) - map * mbm * (up0 - upm - u00 + u0m) - mam * mbp * (u0p - u00 - ump + um0) +
                     mam * mbm * (u00 - u0m - um0 + umm));
}

template <bool VEC>
__global__ __launch_bounds__(256) void bending_bwd_kernel(const float* __restrict__ df, const float* __restrict__ gscale, float coef,
                                                          float* __restrict__ gdf, int D, int H, int W, int zc) {
    constexpr int R = 2, NS = 2 * R + 2;
    using S = Stage<R, VEC>;
    __shared__ __attribute__((aligned(16))) float ring[NS * S::kPlane];
    const float k0 = 2.f * coef * (gscale != nullptr ? gscale[0] : 1.f);
    const Tile t = tile_of_block(D, H, W, zc);
    const float* __restrict__ vol = df + t.vol;
    float* __restrict__ gvol = gdf + t.vol;
    const bool flat = D == 1;
    const int lx = threadIdx.x % kTX, ly = threadIdx.x / kTX;
    const int x = t.x0 + lx;
    const float mxm = inside(x - 1, W), mxc = inside(x, W), mxp = inside(x + 1, W);

    S st;
    {                                                        // planes zb - R .. zb + R into slots 0 .. 2 R: all loads in flight, then the writes
        S pro[2 * R + 1];
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) pro[j].load(vol, t, t.zb - R + j, D, H, W);
        st.load(vol, t, t.zb + R + 1, D, H, W);
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) pro[j].write(ring + j * S::kPlane);
    }
    __syncthreads();

    int base = 0;                                            // slot of plane z - R
    for (int z = t.zb; z < t.ze; ++z) {
        const float* __restrict__ p2m = ring + (base % NS) * S::kPlane;
        const float* __restrict__ p1m = ring + ((base + 1) % NS) * S::kPlane;
        const float* __restrict__ pc = ring + ((base + 2) % NS) * S::kPlane;
        const float* __restrict__ p1p = ring + ((base + 3) % NS) * S::kPlane;
        const float* __restrict__ p2p = ring + ((base + 4) % NS) * S::kPlane;
        // the z mask: 2-D has no z difference (its terms vanish) and every in-plane term counts
        const float mzm = flat ? 0.f : inside(z - 1, D), mzd = flat ? 0.f : inside(z, D), mzp = flat ? 0.f : inside(z + 1, D);
        const float mzc = flat ? 1.f : mzd;
        if (x < W) {
#pragma unroll
            for (int k = 0; k < kTY / kRows; ++k) {
                const int y = t.y0 + ly + kRows * k;
                if (y < H) {
                    const float mym = inside(y - 1, H), myc = inside(y, H), myp = inside(y + 1, H);
                    const int o = (ly + kRows * k + R) * kPitch + lx + kPad;
                    constexpr int P = kPitch;
                    const float c = pc[o];
                    const float xm2 = pc[o - 2], xm1 = pc[o - 1], xp1 = pc[o + 1], xp2 = pc[o + 2];
                    const float ym2 = pc[o - 2 * P], ym1 = pc[o - P], yp1 = pc[o + P], yp2 = pc[o + 2 * P];
                    const float zm2 = p2m[o], zm1 = p1m[o], zp1 = p1p[o], zp2 = p2p[o];
                    float g = myc * mzc * axis_term(xm2, xm1, c, xp1, xp2, mxm, mxc, mxp);
                    g += mxc * mzc * axis_term(ym2, ym1, c, yp1, yp2, mym, myc, myp);
                    g += mxc * myc * axis_term(zm2, zm1, c, zp1, zp2, mzm, mzd, mzp);
                    // (x, y): first index x
                    g += mzc * cross_term(pc[o - 2 - 2 * P], xm2, pc[o - 2 + 2 * P], ym2, c, yp2, pc[o + 2 - 2 * P], xp2, pc[o + 2 + 2 * P],
                                          mxm, mxp, mym, myp);
                    // (x, z)
                    g += myc * cross_term(p2m[o - 2], xm2, p2p[o - 2], zm2, c, zp2, p2m[o + 2], xp2, p2p[o + 2], mxm, mxp, mzm, mzp);
                    // (y, z)
                    g += mxc * cross_term(p2m[o - 2 * P], ym2, p2p[o - 2 * P], zm2, c, zp2, p2m[o + 2 * P], yp2, p2p[o + 2 * P], mym, myp, mzm, mzp);
                    gvol[(long)z * H * W + (y * W + x)] = k0 * g;
                }
            }
        }
        if (z + 1 < t.ze) {
            st.write(ring + ((base + 2 * R + 1) % NS) * S::kPlane);      // plane z + R + 1 over plane z - R - 1 (last read one barrier ago)
            if (z + 2 < t.ze) st.load(vol, t, z + R + 2, D, H, W);
        }
        base = (base + 1) % NS;
        __syncthreads();
    }
}

// workgroups of a launch and the planes per march; 0 workgroups for a shape the kernels do not take (or one whose grid or plane does not fit
// 31 bits)
struct Plan {
    long nblk;
    int zc;
};

inline Plan bending_plan(int64_t nplanes, int D, int H, int W) {
    if (nplanes < 1 || D < 1 || D == 2 || H < 3 || W < 3) return {0, 0};
    if ((long)H * W >= (1L << 31) - 4L * kPitch) return {0, 0};
    const long tiles = (long)nplanes * pulpo::cdiv(H, kTY) * pulpo::cdiv(W, kTX);
    Plan p{0, 0};
    for (int zc : kZC) {
        p = {tiles * pulpo::cdiv(D, zc), zc};
        if (p.nblk >= kMinBlocks) break;
    }
    return p.nblk < (1L << 31) ? p : Plan{0, 0};
}

// rows of whole 16-byte groups (the gradient is stored 4 bytes per lane: its alignment does not matter)
inline bool vec_ok(const float* df, int W) { return (W & 3) == 0 && (reinterpret_cast<uintptr_t>(df) & 15) == 0; }

}  // namespace

// floats of `partial` (= workgroups of either launch); 0: not a shape the kernels take
PULPO_API int pulpo_bending_blocks(int64_t nplanes, int D, int H, int W) { return (int)bending_plan(nplanes, D, H, W).nblk; }

// finish with pulpo_colsum(scale = lamb*D*H*W / (nplanes * max(D-2,1)*(H-2)*(W-2)))
PULPO_API int pulpo_bending_fwd(const float* df, int64_t nplanes, int D, int H, int W, float* partial, void* stream) {
    const Plan pl = bending_plan(nplanes, D, H, W);
    const long nblk = pl.nblk;
    PULPO_REQUIRE(df && partial && nblk > 0, "bending_fwd: bad arguments (non-null pointers, nplanes >= 1, H, W >= 3, D == 1 or D >= 3)");
    if (vec_ok(df, W))
        hipLaunchKernelGGL(bending_fwd_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, df, D, H, W, pl.zc, partial);
    else
        hipLaunchKernelGGL(bending_fwd_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, df, D, H, W, pl.zc, partial);
    return pulpo::check_launch("bending_fwd");
}

PULPO_API int pulpo_bending_bwd(const float* df, const float* gscale, float coef, float* gdf, int64_t nplanes, int D, int H, int W, void* stream) {
    const Plan pl = bending_plan(nplanes, D, H, W);
    const long nblk = pl.nblk;
    PULPO_REQUIRE(df && gdf && nblk > 0, "bending_bwd: bad arguments (non-null pointers, nplanes >= 1, H, W >= 3, D == 1 or D >= 3)");
    if (vec_ok(df, W))
        hipLaunchKernelGGL(bending_bwd_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, df, gscale, coef, gdf, D, H, W, pl.zc);
    else
        hipLaunchKernelGGL(bending_bwd_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, df, gscale, coef, gdf, D, H, W, pl.zc);
    return pulpo::check_launch("bending_bwd");
}
