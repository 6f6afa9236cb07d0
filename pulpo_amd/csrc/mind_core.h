// Per-voxel arithmetic of the MIND-SSC similarity term, shared by the kernels of mind.hip.  Plain C++ without any
// HIP type, so a host program can include it and run the same index arithmetic on the CPU.
//
// Offsets e0..e5 = -z, +z, -y, +y, -x, +x (times the dilation d); channel k is the offset pair (chan_a(k), chan_b(k)):
//   (0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,4) (2,5) (3,4) (3,5)       - the two offsets of a pair lie on different axes
//   S_k(p) = (I(c(p + d e_a)) - I(c(p + d e_b)))^2,  D_k(p) = 1/27 sum_{q in {-1,0,1}^3} S_k(c(p + q)),  c = clamp into the volume
//   m_k = D_k - min_j D_j,  V = mean_k m_k + eps,  f_k = exp(-m_k / V)
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define MIND_HD __host__ __device__ __forceinline__
#else
#define MIND_HD inline
#endif

namespace mind {

constexpr int NCH = 12;

MIND_HD int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
MIND_HD int chan_a(int k) { return k < 4 ? 0 : k < 8 ? 1 : k < 10 ? 2 : 3; }
MIND_HD int chan_b(int k) { return k < 8 ? 2 + (k & 3) : 4 + (k & 1); }
// channel of the offset pair (a, b), a < b on different axes
MIND_HD int chan_of(int a, int b) { return a < 2 ? 4 * a + b - 2 : 8 + 2 * (a - 2) + b - 4; }

// The twelve patch sums 27 D_k of voxel (z,y,x) (the box mean's factor 1/27 is applied in descriptor()) for NI images at once, from a tile that holds the NI images interleaved:
// t[(((gz - oz) * ey + (gy - oy)) * ex + (gx - ox)) * NI + i] = I_i(gz,gy,gx) for every voxel of the volume within d + 1 of the tile's own
// voxels (two images: one 8-byte read serves both).  The box tap is clamped into the volume first and the dilated offset is clamped from
// there, as in the definition: c(c(p + q) + d e), not c(p + q + d e).
template <int NI>
MIND_HD void patch_dist(const float* t, int oz, int oy, int ox, int ey, int ex, int D, int H, int W, int d, int z, int y, int x, float (*Dk)[NCH]) {
    struct alignas(4 * NI) Px { float v[NI]; };
    const Px* tp = reinterpret_cast<const Px*>(t);
    int cx[3], mx[3], px[3];           // per box tap along x: tile offset of the tap, of the tap - d and of the tap + d
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int rx = clampi(x + j - 1, W - 1);
        cx[j] = rx - ox;
        mx[j] = clampi(rx - d, W - 1) - ox;
        px[j] = clampi(rx + d, W - 1) - ox;
    }
    float acc[NI][NCH];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < NCH; ++k) acc[i][k] = 0.f;
    // the nine (z, y) taps as a rolled loop: fully unrolled, the compiler issues all 162 reads ahead of the arithmetic and the kernel
    // needs more than 256 registers per lane
#pragma unroll 1
    for (int j = 0; j < 9; ++j) {
        const int rz = clampi(z + j / 3 - 1, D - 1), ry = clampi(y + j % 3 - 1, H - 1);
        const int cz = (rz - oz) * ey * ex, cy = (ry - oy) * ex;
        const int mz = (clampi(rz - d, D - 1) - oz) * ey * ex, pz = (clampi(rz + d, D - 1) - oz) * ey * ex;
        const int my = (clampi(ry - d, H - 1) - oy) * ex, py = (clampi(ry + d, H - 1) - oy) * ex;
#pragma unroll
        for (int jx = 0; jx < 3; ++jx) {
            Px n[6];
            n[0] = tp[mz + cy + cx[jx]];
            n[1] = tp[pz + cy + cx[jx]];
            n[2] = tp[cz + my + cx[jx]];
            n[3] = tp[cz + py + cx[jx]];
            n[4] = tp[cz + cy + mx[jx]];
            n[5] = tp[cz + cy + px[jx]];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const float df = n[chan_a(k)].v[i] - n[chan_b(k)].v[i];
                    acc[i][k] += df * df;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < NCH; ++k) Dk[i][k] = acc[i][k];
}

// descriptor f_k and its intermediates from the patch sums 27 D_k; returns the arg-min channel (the lowest k on a tie).  The minimum is
// subtracted before the factor 1/27: scaled first, the compiler contracts `sum * (1/27) - min` into one fma, which leaves a rounding residue
// instead of 0 in the arg-min channel, and the descriptor's maximum is then not exactly 1
MIND_HD int descriptor(const float* Dk, float eps, float* f, float* mk, float& V) {
    int am = 0;
    float mn = Dk[0];
#pragma unroll
    for (int k = 1; k < NCH; ++k) {
        if (Dk[k] < mn) {
            mn = Dk[k];
            am = k;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        mk[k] = (Dk[k] - mn) * (1.f / 27.f);
        s += mk[k];
    }
    V = s * (1.f / 12.f) + eps;
#pragma unroll
    for (int k = 0; k < NCH; ++k) f[k] = expf(-mk[k] / V);
    return am;
}

// cost = 1/12 sum_k (fp_k - ft_k)^2
MIND_HD float cost(const float* fp, const float* ft) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const float df = fp[k] - ft[k];
        s += df * df;
    }
    return s * (1.f / 12.f);
}

// G_k = d cost / d D_k[pred]: through f_k = exp(-m_k / V) directly, through V = mean m + eps, and through the minimum to the arg-min channel
MIND_HD void cost_grad(const float* fp, const float* ft, const float* mk, float V, int am, float* G) {
    float a[NCH], sum_afm = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        a[k] = (fp[k] - ft[k]) * (2.f / 12.f) * fp[k];          // d cost / d f_k  *  f_k
        sum_afm += a[k] * mk[k];
    }
    const float rV = 1.f / V, viaV = sum_afm * rV * rV * (1.f / 12.f);
    float sum_b = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        G[k] = viaV - a[k] * rV;                                 // d cost / d m_k
        sum_b += G[k];
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k)
        if (k == am) G[k] -= sum_b;
}

// d loss / d pred(u) as a gather from G (12 planes of one batch item, plane stride N) and the image P of that item:
//   H_k(r) = 1/27 sum over the voxels p whose clamped box tap lands on r of G_k(p)            (adjoint of the clamped 3^3 box)
//   g(u)   = 2 sum_e sum_{r: c(r + d e) = u} sum_{k containing e} H_k(r) (P(u) - P(c(r + d e')))   (e' = the other offset of channel k)
// An interior u has one source r per offset e; a u on a face also collects the r whose offset was clamped onto it, a run of at most d + 1.
MIND_HD float grad_gather(const float* G, long N, const float* P, int D, int H, int W, int d, int z, int y, int x) {
    const int ext[3] = {D, H, W}, u[3] = {z, y, x};
    const int str[3] = {H * W, W, 1};                                // (a volume has fewer than 2^31 voxels)
    const float Pu = P[z * str[0] + y * str[1] + x];
    float total = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const int ax = e >> 1, up = e & 1, n = ext[ax], ua = u[ax];
        int lo, hi;                                                  // the sources' coordinate along ax
        if (up) {
            if (ua == n - 1) { lo = n - 1 - d < 0 ? 0 : n - 1 - d; hi = n - 1; }
            else { lo = hi = ua - d; if (lo < 0) continue; }
        } else {
            if (ua == 0) { lo = 0; hi = d > n - 1 ? n - 1 : d; }
            else { lo = hi = ua + d; if (hi > n - 1) continue; }
        }
        for (int ra = lo; ra <= hi; ++ra) {
            int r[3] = {z, y, x};
            r[ax] = ra;
            int off[3][3];
            float wgt[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int p = r[a] + j - 1;
                    const bool ok = p >= 0 && p < ext[a];
                    // p's taps that land on r[a]: the straight one, and at a face the centre voxel's clamped outward tap as well
                    wgt[a][j] = !ok ? 0.f : (j == 1 && (r[a] == 0 || r[a] == ext[a] - 1)) ? 2.f : 1.f;
                    off[a][j] = clampi(p, ext[a] - 1) * str[a];
                }
            }
            // the four channels that contain e, as a rolled loop (unrolled, their 108 loads are issued together: > 230 registers per lane)
#pragma unroll 1
            for (int e2 = 0; e2 < 6; ++e2) {
                const int ax2 = e2 >> 1;
                if (ax2 == ax) continue;
                const int k = e < e2 ? chan_of(e, e2) : chan_of(e2, e);
                const float* Gk = G + k * N;
                float h = 0.f;
#pragma unroll
                for (int jz = 0; jz < 3; ++jz) {
#pragma unroll
                    for (int jy = 0; jy < 3; ++jy) {
                        const float wzy = wgt[0][jz] * wgt[1][jy];
                        const int ozy = off[0][jz] + off[1][jy];
#pragma unroll
                        for (int jx = 0; jx < 3; ++jx) h += wzy * wgt[2][jx] * Gk[ozy + off[2][jx]];
                    }
                }
                const int sd = (e2 & 1) ? d : -d;                  // the partner offset, clamped from r
                const int o0 = ax2 == 0 ? clampi(r[0] + sd, D - 1) : r[0], o1 = ax2 == 1 ? clampi(r[1] + sd, H - 1) : r[1];
                const int o2 = ax2 == 2 ? clampi(r[2] + sd, W - 1) : r[2];
                total += h * (Pu - P[o0 * str[0] + o1 * str[1] + o2]);
            }
        }
    }
    return total * (2.f / 27.f);
}

}  // namespace mind
