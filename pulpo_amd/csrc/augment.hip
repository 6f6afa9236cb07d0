// On-device training augmentation: a random affine map and a cubic B-spline free-form deformation evaluated once per
// output voxel, and everything that belongs to one sample pulled through that one evaluation.
//   pulpo_augment_apply   image (C channels, trilinear, intensity transform on the way out), mask (float, trilinear) and label map (uint8 /
//                         int32, nearest) of a sample in ONE launch: the sources are read, the results written, and neither a sampling grid
//                         nor a displacement field touches HBM.
//   pulpo_bspline_field   the elastic displacement e, or p - v with an affine on top, as a dense (B,3,D,H,W) tensor: the same tile, the same
//                         headers, the same coordinates bit for bit.
//   pulpo_philox4x32      raw Philox4x32-10 words for given counters (holds the device generator to the published vectors).
// Spatial map: q = v + e(v), p = c + M (q - c) + t (affine_core.h's affine_pos, unchanged).  The sampler works in VOXEL units (it is not
// sampling.h's sample_coord, whose (S-1)-normalised convention does not make a zero displacement the identity): trilinear at p with corners
// outside the volume contributing `fill`, grid_sample(align_corners=True, padding_mode="zeros") for fill = 0; labels at floor(p + 0.5).
// Tile: a workgroup of 256 owns 4 x 4 x 64 voxels (z, y, x), a thread 4 consecutive voxels of a row.  The block's sub-lattice of phi -
// (tile - 1) / s + 5 nodes per axis at most, 3 components - is staged in LDS with nodes outside the lattice as zeros, beside the basis
// values of the tile's 4 + 4 + 64 coordinates (four per axis per voxel, formed once per block) and the log-bias lattice.  A thread sums
// the (z, y) part of the tensor product once per x node (5 nodes cover its 4 voxels: s >= 2) and the x part per voxel.  No atomics.
#include "common.h"
#include "affine_core.h"
#include "bspline_core.h"
#include "philox_core.h"

namespace {

using pulpo::Affine;
using pulpo::affine_load;
using pulpo::affine_pos;

constexpr int TZ = 4, TY = 4, TX = 64, VEC = 4, NT = 256;
constexpr int NCOORD = TZ + TY + TX;
constexpr int kMaxBiasNodes = 4096;
constexpr int kMaxLdsBytes = 64 * 1024;

enum : int { F_GAMMA = 1, F_AFFINE = 2, F_NOISE = 4, F_CLIP = 8 };   // the intensity pieces present (the bias field: a non-null lattice)

struct Tile {
    int z0, y0, x0;      // origin of the block's tile
    int nz, ny, nx;      // extents of the staged sub-lattice
};

__host__ __device__ inline int lat_nodes(int T, int s) { return (T - 1) / s + 5; }

__device__ __forceinline__ Tile tile_of_block(int H, int W, int s) {
    const int ntx = (W + TX - 1) / TX, nty = (H + TY - 1) / TY;
    int t = blockIdx.x;
    Tile T;
    T.x0 = (t % ntx) * TX;
    t /= ntx;
    T.y0 = (t % nty) * TY;
    T.z0 = (t / nty) * TZ;
    T.nz = lat_nodes(TZ, s);
    T.ny = lat_nodes(TY, s);
    T.nx = lat_nodes(TX, s);
    return T;
}

// LDS layout (floats): wtab[NCOORD][4] | ctab[NCOORD] (ints) | lat[3][nz][ny][nx] | bias[Lz Ly Lx]
__host__ __device__ inline int lds_lat_offset() { return NCOORD * 5; }
inline size_t lds_bytes(int s, bool has_phi, int nbias) {
    const size_t lat = has_phi ? (size_t)3 * lat_nodes(TZ, s) * lat_nodes(TY, s) * lat_nodes(TX, s) : 0;
    return (lds_lat_offset() + lat + nbias) * sizeof(float);
}

// basis values and relative cells of the tile's coordinates, and the sub-lattice of phi[b]; ends with a barrier
__device__ __forceinline__ void stage_lattice(float* __restrict__ lds, const Tile& T, const float* __restrict__ phib, int s, int D, int H, int W, int Gz, int Gy,
                                              int Gx) {
    float* wtab = lds;
    int* ctab = reinterpret_cast<int*>(lds + NCOORD * 4);
    float* lat = lds + lds_lat_offset();
    const int iz0 = D == 1 ? 0 : T.z0 / s, iy0 = T.y0 / s, ix0 = T.x0 / s;
    const int t = threadIdx.x;
    if (t < NCOORD) {
        int v, i0;
        bool one = false;
        if (t < TZ) { v = T.z0 + t; i0 = iz0; one = D == 1; }
        else if (t < TZ + TY) { v = T.y0 + t - TZ; i0 = iy0; }
        else { v = T.x0 + t - TZ - TY; i0 = ix0; }
        float w[4];
        const int i = pulpo::bspline_weights(v, s, one, w);
        wtab[4 * t] = w[0]; wtab[4 * t + 1] = w[1]; wtab[4 * t + 2] = w[2]; wtab[4 * t + 3] = w[3];
        ctab[t] = i - i0;
    }
    const int nyx = T.ny * T.nx, n = T.nz * nyx;
    const long G = (long)Gz * Gy * Gx;
    for (int e = t; e < 3 * n; e += NT) {
        const int a = e / n, r = e - a * n;
        const int lz = r / nyx, r2 = r - lz * nyx, ly = r2 / T.nx, lx = r2 - ly * T.nx;
        const int gz = iz0 + lz, gy = iy0 + ly, gx = ix0 + lx;
        lat[e] = (gz < Gz && gy < Gy && gx < Gx) ? phib[a * G + ((long)gz * Gy + gy) * Gx + gx] : 0.f;     // (nodes past the lattice: zeros)
    }
    __syncthreads();
}

// e[a][k]: the elastic displacement of the thread's VEC voxels (row (tz, ty), x group tx of the tile) from the staged lattice
__device__ __forceinline__ void elastic_of_thread(const float* __restrict__ lds, const Tile& T, int tz, int ty, int tx, float e[3][VEC]) {
    const float* wtab = lds;
    const int* ctab = reinterpret_cast<const int*>(lds + NCOORD * 4);
    const float* lat = lds + lds_lat_offset();
    const int cz = ctab[tz], cy = ctab[TZ + ty], xe = TZ + TY + VEC * tx, cx0 = ctab[xe];
    float wzy[16];
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int m = 0; m < 4; ++m) wzy[4 * l + m] = wtab[4 * tz + l] * wtab[4 * (TZ + ty) + m];
    const int nyx = T.ny * T.nx, n = T.nz * nyx;
    const bool two = ctab[xe + VEC - 1] != cx0;                  // the four voxels lie in two cells (never more: s >= 2): a fifth x node
    float col[3][5];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float* node = lat + a * n + (cz * T.ny + cy) * T.nx + cx0;
#pragma unroll
        for (int j = 0; j < 4; ++j) col[a][j] = pulpo::bspline_column(node + j, nyx, T.nx, wzy);
        col[a][4] = two ? pulpo::bspline_column(node + 4, nyx, T.nx, wzy) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const bool up = ctab[xe + k] != cx0;
        float wx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wx[j] = wtab[4 * (xe + k) + j];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float cc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cc[j] = up ? col[a][j + 1] : col[a][j];
            e[a][k] = pulpo::bspline_row(wx, cc);
        }
    }
}

// p[a][k] of the thread's voxels: q = v + e, then the affine; a depth-1 grid has no depth coordinate (p_z = 0)
__device__ __forceinline__ void positions_of_thread(const float* __restrict__ lds, const Tile& T, bool has_phi, const float* __restrict__ thetab, int tz, int ty,
                                                    int tx, int D, int H, int W, float p[3][VEC], float e[3][VEC]) {
    const int z = T.z0 + tz, y = T.y0 + ty, x = T.x0 + VEC * tx;
    if (has_phi) {
        elastic_of_thread(lds, T, tz, ty, tx, e);
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < VEC; ++k) e[a][k] = 0.f;
    }
    if (D == 1) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) e[0][k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        p[0][k] = (float)z + e[0][k];
        p[1][k] = (float)y + e[1][k];
        p[2][k] = (float)(x + k) + e[2][k];
    }
    if (thetab) {
        const Affine A = affine_load(thetab, D, H, W);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float r[3];
            affine_pos(A, p[0][k], p[1][k], p[2][k], r);
            p[0][k] = D == 1 ? 0.f : r[0];
            p[1][k] = r[1];
            p[2][k] = r[2];
        }
    }
}

// one axis of the voxel-unit sampler: corner i0 = floor(p), weight f of corner i0 + 1; positions two voxels and more outside the volume
// are pulled to there first (every corner is still outside, and the conversion to int stays defined for any p, a NaN included)
struct Axis {
    int i0;
    float f;
};

__device__ __forceinline__ float pull_in(float p, int S) { return fminf(fmaxf(p, -2.f), (float)S + 1.f); }

__device__ __forceinline__ Axis axis_of(float p, int S) {
    const float q = pull_in(p, S), fl = floorf(q);
    Axis a;
    a.i0 = (int)fl;
    a.f = q - fl;
    return a;
}

__device__ __forceinline__ float corner(const float* __restrict__ s, int z, int y, int x, int D, int H, int W, float fill) {
    const bool in = (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    return in ? s[((long)z * H + y) * W + x] : fill;
}

__device__ __forceinline__ float trilinear(const float* __restrict__ s, const Axis& az, const Axis& ay, const Axis& ax, int D, int H, int W, float fill) {
    const float s000 = corner(s, az.i0, ay.i0, ax.i0, D, H, W, fill), s001 = corner(s, az.i0, ay.i0, ax.i0 + 1, D, H, W, fill);
    const float s010 = corner(s, az.i0, ay.i0 + 1, ax.i0, D, H, W, fill), s011 = corner(s, az.i0, ay.i0 + 1, ax.i0 + 1, D, H, W, fill);
    const float s100 = corner(s, az.i0 + 1, ay.i0, ax.i0, D, H, W, fill), s101 = corner(s, az.i0 + 1, ay.i0, ax.i0 + 1, D, H, W, fill);
    const float s110 = corner(s, az.i0 + 1, ay.i0 + 1, ax.i0, D, H, W, fill), s111 = corner(s, az.i0 + 1, ay.i0 + 1, ax.i0 + 1, D, H, W, fill);
    const float wz0 = 1.f - az.f, wy0 = 1.f - ay.f, wx0 = 1.f - ax.f;
    return wz0 * wy0 * wx0 * s000 + wz0 * wy0 * ax.f * s001 + wz0 * ay.f * wx0 * s010 + wz0 * ay.f * ax.f * s011 + az.f * wy0 * wx0 * s100 +
           az.f * wy0 * ax.f * s101 + az.f * ay.f * wx0 * s110 + az.f * ay.f * ax.f * s111;
}

__device__ __forceinline__ int nearest(float p, int S) { return (int)floorf(pull_in(p, S) + 0.5f); }

// one axis of the log-bias lattice, whose end nodes sit on the volume's end voxels: node i0 and the weight of node i1
__device__ __forceinline__ void bias_axis(int v, int S, int L, int& i0, int& i1, float& f) {
    const float g = (S > 1 && L > 1) ? (float)v * ((float)(L - 1) / (float)(S - 1)) : 0.f;
    i0 = min((int)g, max(L - 2, 0));
    i1 = min(i0 + 1, L - 1);
    f = g - (float)i0;
}

template <typename T>
__device__ __forceinline__ void store_vec(T* __restrict__ o, const T r[VEC], bool vec, int x, int W) {
    if (vec) {
        if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(r);
        else *reinterpret_cast<uint32_t*>(o) = *reinterpret_cast<const uint32_t*>(r);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (x + k < W) o[k] = r[k];
    }
}

template <typename L>
__device__ __forceinline__ void gather_labels(const L* __restrict__ src, L* __restrict__ dst, const float p[3][VEC], int fill_label, bool vec, int x, int D, int H,
                                              int W) {
    alignas(16) L r[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int iz = nearest(p[0][k], D), iy = nearest(p[1][k], H), ix = nearest(p[2][k], W);
        const bool in = (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        r[k] = in ? src[((long)iz * H + iy) * W + ix] : (L)fill_label;
    }
    store_vec(dst, r, vec, x, W);
}

struct AugmentArgs {
    const float* theta;      // (B,3,4) or null: the identity
    const float* phi;        // (B,3,Gz,Gy,Gx) or null: e = 0
    const float* img;        // (B,C,D,H,W) or null
    float* img_out;
    const float* mask;       // (B,Cm,D,H,W) or null
    float* mask_out;
    const void* labels;      // (B,1,D,H,W) uint8 / int32 or null
    void* labels_out;
    const float* iparams;    // (B,4): gamma, gain, offset, sigma
    const float* bias;       // (B,Lz,Ly,Lx) or null
    const uint32_t* seed;    // two words on the device: lo, hi
    int s, Gz, Gy, Gx, C, Cm, ldt, iflags, Lz, Ly, Lx;
    float fill;
    int fill_label, D, H, W;
    int vec_img, vec_mask, vec_lab;
};

__global__ __launch_bounds__(NT) void augment_apply_kernel(const AugmentArgs P) {
    extern __shared__ __align__(16) float lds[];
    const int b = blockIdx.y, D = P.D, H = P.H, W = P.W;
    const Tile T = tile_of_block(H, W, P.s);
    const bool has_phi = P.phi != nullptr;
    const long V = (long)D * H * W;
    const int nlat = has_phi ? 3 * T.nz * T.ny * T.nx : 0;
    float* sbias = lds + lds_lat_offset() + nlat;
    const int nbias = P.bias ? P.Lz * P.Ly * P.Lx : 0;
    for (int e = threadIdx.x; e < nbias; e += NT) sbias[e] = P.bias[(long)b * nbias + e];
    if (has_phi) stage_lattice(lds, T, P.phi + (long)b * 3 * P.Gz * P.Gy * P.Gx, P.s, D, H, W, P.Gz, P.Gy, P.Gx);
    else __syncthreads();

    const int tx = threadIdx.x & 15, ty = (threadIdx.x >> 4) & 3, tz = threadIdx.x >> 6;
    const int z = T.z0 + tz, y = T.y0 + ty, x = T.x0 + VEC * tx;
    if (z >= D || y >= H || x >= W) return;                      // (after the only barrier)
    float p[3][VEC], e[3][VEC];
    positions_of_thread(lds, T, has_phi, P.theta ? P.theta + (long)b * 12 : nullptr, tz, ty, tx, D, H, W, p, e);
    const long v0 = ((long)z * H + y) * W + x;

    if (P.labels) {
        if (P.ldt == 0)
            gather_labels((const uint8_t*)P.labels + b * V, (uint8_t*)P.labels_out + b * V + v0, p, P.fill_label, P.vec_lab != 0, x, D, H, W);
        else
            gather_labels((const int*)P.labels + b * V, (int*)P.labels_out + b * V + v0, p, P.fill_label, P.vec_lab != 0, x, D, H, W);
    }
    if (!P.img && !P.mask) return;

    Axis az[VEC], ay[VEC], ax[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        az[k] = axis_of(p[0][k], D);
        ay[k] = axis_of(p[1][k], H);
        ax[k] = axis_of(p[2][k], W);
    }
    if (P.mask) {
        for (int c = 0; c < P.Cm; ++c) {
            const float* s = P.mask + ((long)b * P.Cm + c) * V;
            alignas(16) float r[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] = trilinear(s, az[k], ay[k], ax[k], D, H, W, P.fill);
            store_vec(P.mask_out + ((long)b * P.Cm + c) * V + v0, r, P.vec_mask != 0, x, W);
        }
    }
    if (!P.img) return;

    float gamma = 1.f, gain = 1.f, offset = 0.f, sigma = 0.f;
    if (P.iparams) {
        gamma = P.iparams[4 * b];
        gain = P.iparams[4 * b + 1];
        offset = P.iparams[4 * b + 2];
        sigma = P.iparams[4 * b + 3];
    }
    float gainf[VEC];                                            // exp(beta(v)), the multiplicative bias field
    if (P.bias) {
        int z0i, z1i, y0i, y1i;
        float fz, fy;
        bias_axis(z, D, P.Lz, z0i, z1i, fz);
        bias_axis(y, H, P.Ly, y0i, y1i, fy);
        const float* r00 = sbias + (z0i * P.Ly + y0i) * P.Lx;
        const float* r01 = sbias + (z0i * P.Ly + y1i) * P.Lx;
        const float* r10 = sbias + (z1i * P.Ly + y0i) * P.Lx;
        const float* r11 = sbias + (z1i * P.Ly + y1i) * P.Lx;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            int x0i, x1i;
            float fx;
            bias_axis(x + k, W, P.Lx, x0i, x1i, fx);
            const float b00 = __fmaf_rn(fx, r00[x1i] - r00[x0i], r00[x0i]), b01 = __fmaf_rn(fx, r01[x1i] - r01[x0i], r01[x0i]);
            const float b10 = __fmaf_rn(fx, r10[x1i] - r10[x0i], r10[x0i]), b11 = __fmaf_rn(fx, r11[x1i] - r11[x0i], r11[x0i]);
            const float b0 = __fmaf_rn(fy, b01 - b00, b00), b1 = __fmaf_rn(fy, b11 - b10, b10);
            gainf[k] = expf(__fmaf_rn(fz, b1 - b0, b0));
        }
    }
    uint32_t seed_lo = 0, seed_hi = 0;
    if (P.iflags & F_NOISE) {
        seed_lo = P.seed[0];
        seed_hi = P.seed[1];
    }
    for (int c = 0; c < P.C; ++c) {
        const long plane = ((long)b * P.C + c) * V;
        const float* s = P.img + plane;
        alignas(16) float r[VEC];
        pulpo::Philox4 words;
        uint64_t group = ~(uint64_t)0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float t = trilinear(s, az[k], ay[k], ax[k], D, H, W, P.fill);
            if (P.iflags & F_GAMMA) t = powf(fminf(fmaxf(t, 0.f), 1.f), gamma);
            if (P.bias) t *= gainf[k];
            if (P.iflags & F_AFFINE) t = __fmaf_rn(gain, t, offset);
            if (P.iflags & F_NOISE) {
                const uint64_t i = (uint64_t)(plane + v0 + k);
                if ((i >> 2) != group) {
                    group = i >> 2;
                    words = pulpo::philox_group(group, seed_lo, seed_hi);
                }
                t = __fmaf_rn(sigma, pulpo::philox_normal(words, (int)(i & 3)), t);
            }
            if (P.iflags & F_CLIP) t = fminf(fmaxf(t, 0.f), 1.f);
            r[k] = t;
        }
        store_vec(P.img_out + plane + v0, r, P.vec_img != 0, x, W);
    }
}

__global__ __launch_bounds__(NT) void bspline_field_kernel(const float* __restrict__ phi, const float* __restrict__ theta, float* __restrict__ out, int s, int Gz,
                                                           int Gy, int Gx, int D, int H, int W, int vec) {
    extern __shared__ __align__(16) float lds[];
    const int b = blockIdx.y;
    const Tile T = tile_of_block(H, W, s);
    stage_lattice(lds, T, phi + (long)b * 3 * Gz * Gy * Gx, s, D, H, W, Gz, Gy, Gx);
    const int tx = threadIdx.x & 15, ty = (threadIdx.x >> 4) & 3, tz = threadIdx.x >> 6;
    const int z = T.z0 + tz, y = T.y0 + ty, x = T.x0 + VEC * tx;
    if (z >= D || y >= H || x >= W) return;
    float p[3][VEC], e[3][VEC];
    positions_of_thread(lds, T, true, theta ? theta + (long)b * 12 : nullptr, tz, ty, tx, D, H, W, p, e);
    const long V = (long)D * H * W, v0 = ((long)z * H + y) * W + x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        alignas(16) float r[VEC];
        const float va[3] = {(float)z, (float)y, (float)x};
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float v = a == 2 ? (float)(x + k) : va[a];
            r[k] = (a == 0 && D == 1) ? 0.f : (theta ? p[a][k] - v : e[a][k]);     // e itself without an affine: (v + e) - v would round it
        }
        store_vec(out + ((long)b * 3 + a) * V + v0, r, vec != 0, x, W);
    }
}

__global__ __launch_bounds__(NT) void philox_kernel(const uint32_t* __restrict__ counters, const uint32_t* __restrict__ key, uint32_t* __restrict__ out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const pulpo::Philox4 w = pulpo::philox4x32_10(counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3], key[0], key[1]);
        out[4 * i] = w.r[0];
        out[4 * i + 1] = w.r[1];
        out[4 * i + 2] = w.r[2];
        out[4 * i + 3] = w.r[3];
    }
}

inline bool rows4(int W, const void* a, size_t align) { return W % 4 == 0 && (((uintptr_t)a) & (align - 1)) == 0; }

inline long tiles(int D, int H, int W) { return (long)pulpo::cdiv(D, TZ) * pulpo::cdiv(H, TY) * pulpo::cdiv(W, TX); }

inline bool lattice_fits(int S, int G, int s) { return G == (S - 1 + s - 1) / s + 3; }

}  // namespace

PULPO_API int pulpo_augment_apply(const float* theta, const float* phi, int spacing, int Gz, int Gy, int Gx, const float* img, float* img_out, int C,
                                  const float* mask, float* mask_out, int Cm, const void* labels, void* labels_out, int ldt, const float* iparams, int iflags,
                                  const float* bias, int Lz, int Ly, int Lx, const void* seed, float fill, int fill_label, int B, int D, int H, int W,
                                  void* stream) {
    PULPO_REQUIRE(img || mask || labels, "augment_apply: no source");
    PULPO_REQUIRE((!img || (img_out && C >= 1)) && (!mask || (mask_out && Cm >= 1)) && (!labels || (labels_out && (ldt == 0 || ldt == 1))),
                  "augment_apply: every source needs its output (C, Cm >= 1; ldt 0 uint8 or 1 int32)");
    PULPO_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long)D * H * W < (1L << 31), "augment_apply: B >= 1 and extents >= 1 (fewer than 2^31 voxels) expected");
    PULPO_REQUIRE(tiles(D, H, W) < (1L << 31), "augment_apply: too many tiles");
    if (phi) {
        PULPO_REQUIRE(spacing >= 2, "augment_apply: lattice spacing >= 2 expected");
        PULPO_REQUIRE((D == 1 ? Gz == 1 : lattice_fits(D, Gz, spacing)) && lattice_fits(H, Gy, spacing) && lattice_fits(W, Gx, spacing),
                      "augment_apply: lattice extents ceil((S - 1) / s) + 3 per axis expected (1 along a depth-1 axis)");
    } else {
        spacing = 2;
    }
    PULPO_REQUIRE((iflags & ~(F_GAMMA | F_AFFINE | F_NOISE | F_CLIP)) == 0, "augment_apply: unknown intensity flag");
    PULPO_REQUIRE(!(iflags & (F_GAMMA | F_AFFINE | F_NOISE)) || iparams, "augment_apply: gamma, gain / offset and sigma come in iparams (B,4)");
    PULPO_REQUIRE(!(iflags & F_NOISE) || seed, "augment_apply: noise needs a seed on the device");
    int nbias = 0;
    if (bias) {
        PULPO_REQUIRE(Lz >= 1 && Ly >= 1 && Lx >= 1 && (long)Lz * Ly * Lx <= kMaxBiasNodes, "augment_apply: a bias lattice of 1 to 4096 nodes expected");
        nbias = Lz * Ly * Lx;
    }
    const size_t shm = lds_bytes(spacing, phi != nullptr, nbias);
    PULPO_REQUIRE(shm <= (size_t)kMaxLdsBytes, "augment_apply: the staged lattices exceed 64 KiB of LDS");
    AugmentArgs P;
    P.theta = theta; P.phi = phi; P.img = img; P.img_out = img_out; P.mask = mask; P.mask_out = mask_out; P.labels = labels; P.labels_out = labels_out;
    P.iparams = iparams; P.bias = bias; P.seed = (const uint32_t*)seed;
    P.s = spacing; P.Gz = Gz; P.Gy = Gy; P.Gx = Gx; P.C = C; P.Cm = Cm; P.ldt = ldt; P.iflags = img ? iflags : 0; P.Lz = Lz; P.Ly = Ly; P.Lx = Lx;
    P.fill = fill; P.fill_label = fill_label; P.D = D; P.H = H; P.W = W;
    P.vec_img = img && rows4(W, img_out, 16);
    P.vec_mask = mask && rows4(W, mask_out, 16);
    P.vec_lab = labels && rows4(W, labels_out, ldt == 0 ? 4 : 16);
    hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)tiles(D, H, W), B), dim3(NT), shm, (hipStream_t)stream, P);
    return pulpo::check_launch("augment_apply");
}

PULPO_API int pulpo_bspline_field(const float* phi, const float* theta, float* out, int spacing, int Gz, int Gy, int Gx, int B, int D, int H, int W,
                                  void* stream) {
    PULPO_REQUIRE(phi && out, "bspline_field: null pointer");
    PULPO_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long)D * H * W < (1L << 31), "bspline_field: B >= 1 and extents >= 1 (fewer than 2^31 voxels) expected");
    PULPO_REQUIRE(spacing >= 2, "bspline_field: lattice spacing >= 2 expected");
    PULPO_REQUIRE((D == 1 ? Gz == 1 : lattice_fits(D, Gz, spacing)) && lattice_fits(H, Gy, spacing) && lattice_fits(W, Gx, spacing),
                  "bspline_field: lattice extents ceil((S - 1) / s) + 3 per axis expected (1 along a depth-1 axis)");
    const size_t shm = lds_bytes(spacing, true, 0);
    PULPO_REQUIRE(shm <= (size_t)kMaxLdsBytes, "bspline_field: the staged lattice exceeds 64 KiB of LDS");
    hipLaunchKernelGGL(bspline_field_kernel, dim3((unsigned)tiles(D, H, W), B), dim3(NT), shm, (hipStream_t)stream, phi, theta, out, spacing, Gz, Gy, Gx, D, H, W,
                       (int)rows4(W, out, 16));
    return pulpo::check_launch("bspline_field");
}

PULPO_API int pulpo_philox4x32(const void* counters, const void* key, void* out, int64_t n, void* stream) {
    PULPO_REQUIRE(counters && key && out && n >= 1, "philox4x32: null pointer or n < 1");
    hipLaunchKernelGGL(philox_kernel, dim3(pulpo::eblocks(n, 2048)), dim3(NT), 0, (hipStream_t)stream, (const uint32_t*)counters, (const uint32_t*)key,
                       (uint32_t*)out, (long)n);
    return pulpo::check_launch("philox4x32");
}
