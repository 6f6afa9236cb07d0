// Tile-level pieces of the forward / data-gradient convolution kernels.  For all of them (conv3d.hip, conv3d_bf16.hip, conv3d_wino.hip,
// conv3d_wino2p.hip, conv3d_wino3.hip): the decode of a linear work id into a voxel tile and the statistics store that sums the waves' rows.
// For the Winograd kernels: the epilogue in the float4 form their fast paths use - a lane holds four channels of two voxels (v0, v1 - the even
// and the odd output of the last inverse-transform step) - and, for the two F(2x2,3x3) kernels, the pieces of the tile epilogue body.  Where a
// kernel keeps a piece as its own text (the call made its register allocation worse), a comment there names the function it mirrors.
// ONE definition each, as sampling.h does for the warp coordinate: the three kernels' statistics rows and stored values are held to the same
// bits by the suite (the fused-against-separate tests), and a change to the epilogue is made in one place.  The per-element expressions
// themselves are head_bn.h's (bn_lrelu, bn_bwd_reduce_step), shared with norm_act.hip and heads.hip.  Device inline functions only.
#pragma once
#include "conv_shared.h"
#include "head_bn.h"

namespace pulpo_conv {

// work item -> (cout tile, voxel tile): work = tile_lin * ncot + cot, tile_lin = ((b * ntz + tz) * nty + ty) * ntx + tx (the row of the
// statistics buffer); tz: the tile's z extent, NT: couts per tile.  Args: ConvArgs or the bf16 kernels' argument block (same field names)
struct TileId { int tile_lin, b, z0, y0, x0, co0; };
template <typename Args>
__device__ __forceinline__ TileId decode_tile(const Args& a, int work, int tz, int nt) {
    TileId t;
    const int cot = work % a.ncot;
    t.tile_lin = work / a.ncot;
    int q = t.tile_lin;
    const int tx_ = q % a.ntx; q /= a.ntx;
    const int ty_ = q % a.nty; q /= a.nty;
    const int tz_ = q % a.ntz;
    t.b = q / a.ntz;
    t.z0 = tz_ * tz; t.y0 = ty_ * TY; t.x0 = tx_ * TX;
    t.co0 = cot * nt;
    return t;
}

// per-tile BatchNorm partial sums: the NW waves' rows red[wave][2][NT] added in wave order by threads 0 .. 2 NT - 1 and stored to
// stats[tile][2][Cout] (channels of a partly empty cout tile are skipped).  The rows are sums that started from +0, so no row is -0 and
// "row 0 first" equals "0 + row 0".  FULL: the kernel runs with full cout tiles only, no channel check.  The caller has passed the barrier
// behind the rows' stores.  on: block-uniform (statistics asked for, a tile pending), one condition with the thread test.
template <int NW, int NT, bool FULL = false>
__device__ __forceinline__ void stats_store(bool on, const float* red, float* __restrict__ stats, int tile_lin, int Cout, int co0, int tid) {
    if (on && tid < 2 * NT) {
        const int which = tid / NT, c = tid - which * NT;
        if (FULL || co0 + c < Cout) {
            float tot = red[which * NT + c];
#pragma unroll
            for (int w = 1; w < NW; ++w) tot += red[(w * 2 + which) * NT + c];
            stats[((long)tile_lin * 2 + which) * Cout + co0 + c] = tot;
        }
    }
}

// fast path of the F(2x2,3x3) kernels, lane = (channel quad q, row half, row group): sum over the lanes that hold the same four channels
// (xor 8, 16, 32), lanes 0 - 7 store the wave's rows red[wave][0 | 1][4 q ..]
template <int NT>
__device__ __forceinline__ void quad_reduce_to_red(float4 s4, float4 q4, float* red, int wave, int elane) {
#pragma unroll
    for (int o = 8; o <= 32; o <<= 1) {
        s4.x += __shfl_xor(s4.x, o, 64); s4.y += __shfl_xor(s4.y, o, 64); s4.z += __shfl_xor(s4.z, o, 64); s4.w += __shfl_xor(s4.w, o, 64);
        q4.x += __shfl_xor(q4.x, o, 64); q4.y += __shfl_xor(q4.y, o, 64); q4.z += __shfl_xor(q4.z, o, 64); q4.w += __shfl_xor(q4.w, o, 64);
    }
    if (elane < 8) {
        *reinterpret_cast<float4*>(red + (wave * 2 + 0) * NT + 4 * elane) = s4;
        *reinterpret_cast<float4*>(red + (wave * 2 + 1) * NT + 4 * elane) = q4;
    }
}

// general path: lane = (row half, channel i): sum of the two halves, lanes 0 - 31 store the wave's rows
template <int NT>
__device__ __forceinline__ void half_reduce_to_red(float ssum, float ssq, float* red, int wave, int elane) {
    ssum += __shfl_xor(ssum, 32, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    if (elane < 32) {
        red[(wave * 2 + 0) * NT + elane] = ssum;
        red[(wave * 2 + 1) * NT + elane] = ssq;
    }
}

// last step of the F(2,3) inverse transform with the bias: v0 = t0 + t1 + t2 + b, v1 = t1 - t2 - t3 + b
__device__ __forceinline__ void inverse_last(const float4& t0, const float4& t1, const float4& t2, const float4& t3, const float4& b4, float4& v0, float4& v1) {
    v0 = make_float4(t0.x + t1.x + t2.x + b4.x, t0.y + t1.y + t2.y + b4.y, t0.z + t1.z + t2.z + b4.z, t0.w + t1.w + t2.w + b4.w);
    v1 = make_float4(t1.x - t2.x - t3.x + b4.x, t1.y - t2.y - t3.y + b4.y, t1.z - t2.z - t3.z + b4.z, t1.w - t2.w - t3.w + b4.w);
}

// BatchNorm statistics of a whole voxel pair: s4 += v0 + v1, q4 += v0^2 + v1^2
__device__ __forceinline__ void stats_add_pair(const float4& v0, const float4& v1, float4& s4, float4& q4) {
    s4.x += v0.x + v1.x; s4.y += v0.y + v1.y; s4.z += v0.z + v1.z; s4.w += v0.w + v1.w;
    q4.x += v0.x * v0.x + v1.x * v1.x; q4.y += v0.y * v0.y + v1.y * v1.y; q4.z += v0.z * v0.z + v1.z * v1.z; q4.w += v0.w * v0.w + v1.w * v1.w;
}

// ... of one voxel (the masked form: the pipelined kernel's ragged tiles)
__device__ __forceinline__ void stats_add_one(const float4& v, float4& s4, float4& q4) {
    s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
    q4.x += v.x * v.x; q4.y += v.y * v.y; q4.z += v.z * v.z; q4.w += v.w * v.w;
}

// first BatchNorm-backward pass over the eight values of a voxel pair (dz = v0 | v1, pre-norm activations y0 | y1): pulpo::bn_bwd_reduce_step
__device__ __forceinline__ void bn_bwd_reduce_pair(const float4& v0, const float4& v1, const float4& y0, const float4& y1, const float4& sc4, const float4& sh4,
                                                   const float4& m4, float slope, float4& s4, float4& q4) {
    pulpo::bn_bwd_reduce_step(v0.x, y0.x, sc4.x, sh4.x, m4.x, slope, s4.x, q4.x);
    pulpo::bn_bwd_reduce_step(v0.y, y0.y, sc4.y, sh4.y, m4.y, slope, s4.y, q4.y);
    pulpo::bn_bwd_reduce_step(v0.z, y0.z, sc4.z, sh4.z, m4.z, slope, s4.z, q4.z);
    pulpo::bn_bwd_reduce_step(v0.w, y0.w, sc4.w, sh4.w, m4.w, slope, s4.w, q4.w);
    pulpo::bn_bwd_reduce_step(v1.x, y1.x, sc4.x, sh4.x, m4.x, slope, s4.x, q4.x);
    pulpo::bn_bwd_reduce_step(v1.y, y1.y, sc4.y, sh4.y, m4.y, slope, s4.y, q4.y);
    pulpo::bn_bwd_reduce_step(v1.z, y1.z, sc4.z, sh4.z, m4.z, slope, s4.z, q4.z);
    pulpo::bn_bwd_reduce_step(v1.w, y1.w, sc4.w, sh4.w, m4.w, slope, s4.w, q4.w);
}

// eval-mode fused store: pulpo::bn_lrelu on four channels
__device__ __forceinline__ float4 bn_lrelu4(const float4& v, const float4& sc4, const float4& sh4, float slope) {
    return make_float4(pulpo::bn_lrelu(v.x, sc4.x, sh4.x, slope), pulpo::bn_lrelu(v.y, sc4.y, sh4.y, slope), pulpo::bn_lrelu(v.z, sc4.z, sh4.z, slope),
                       pulpo::bn_lrelu(v.w, sc4.w, sh4.w, slope));
}

// ---- the tile epilogue of the two F(2x2,3x3) kernels (conv3d_wino.hip, conv3d_wino2p.hip): x inverse transform in registers, y inverse transform
// across the four waves through the exchange buffer R = [py][ox][r][lane], one row tile m (two z-planes) at a time.  Barriers stay with the kernels.
// Lane roles: fast path lane = (channel quad q = lane & 7, row half kh = (lane >> 3) & 1, row group g = lane >> 4); general path lane = (row
// half lane >> 5, channel lane & 31) - that path stays kernel text, see there.

// wave py's x-inverse-transformed partial rows of row tile m into the exchange buffer
__device__ __forceinline__ void wino2_exchange_write(float* R, const f32x16 (&acc)[4], int py, int elane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float m0 = acc[0][r], m1 = acc[1][r], m2 = acc[2][r], m3 = acc[3][r];
        R[((py * 2 + 0) * 16 + r) * 64 + elane] = m0 + m1 + m2;
        R[((py * 2 + 1) * 16 + r) * 64 + elane] = m1 - m2 - m3;
    }
}

// the voxel pair (y, y + 1) a fast-path lane finishes in half h of row tile m: its (ox, r) slot of the exchange buffer and its coordinates
struct Wino2Voxel { int ox, r, gz, gy, gx; long vox; };
__device__ __forceinline__ Wino2Voxel wino2_voxel(const ConvArgs& a, int h, int m, int wave, int g, int kh, int z0, int y0, int x0) {
    Wino2Voxel v;
    const int combo = h * 16 + wave * 4 + g;
    v.ox = combo >> 4; v.r = combo & 15;
    const int row = (v.r & 3) + 8 * (v.r >> 2) + 4 * kh;
    v.gz = z0 + 2 * m + (row >> 4); v.gy = y0 + 2 * ((row >> 2) & 3); v.gx = x0 + 2 * (row & 3) + v.ox;
    v.vox = (long)(v.gz * a.H + v.gy) * a.W + v.gx;
    return v;
}

// (BatchNorm-backward reduction) the pre-norm activations of the lane's four voxels; bn_b: batch element, channel co0 + 4 q
__device__ __forceinline__ void wino2_load_y(float4 (&yv)[2][2], const ConvArgs& a, const float* bn_b, int m, int wave, int g, int kh, int z0, int y0, int x0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const Wino2Voxel v = wino2_voxel(a, h, m, wave, g, kh, z0, y0, x0);
        yv[h][0] = *reinterpret_cast<const float4*>(bn_b + v.vox * a.bn_y_ps);
        yv[h][1] = *reinterpret_cast<const float4*>(bn_b + (v.vox + a.W) * a.bn_y_ps);
    }
}

// fast path: the four waves' partial rows by ds_read_b128 (all issued before the first use), the y inverse transform on float4s, each voxel
// leaves as one 128-byte line written by 8 lanes x 16 bytes.  whole: the tile lies inside the volume (the round-2 kernel takes this path on
// whole tiles only and passes `true`: the edge masks fold away); out_b: batch element; bnr: s4 / q4 receive the
// BatchNorm-backward sums (yv, sc4, sh4, bm4 of the unit in front) instead of sum and sum of squares; fuse: eval-mode store with sc4 / sh4
__device__ __forceinline__ void wino2_fast_path(const float* R, float* out_b, long o_ps, int co0, const ConvArgs& a, int m, int wave, int g, int kh, int q, int z0, int y0,
                                                int x0, bool whole, bool bnr, bool fuse, const float4& b4, const float4& sc4, const float4& sh4, const float4& bm4,
                                                const float4 (&yv)[2][2], float4& s4, float4& q4) {
    float4 tq[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int combo = h * 16 + wave * 4 + g;               // (ox, r) = (combo >> 4, combo & 15)
#pragma unroll
        for (int p = 0; p < 4; ++p)
            tq[h][p] = *reinterpret_cast<const float4*>(R + ((p * 2 + (combo >> 4)) * 16 + (combo & 15)) * 64 + kh * 32 + 4 * q);
    }
    float* obase = out_b + co0 + 4 * q;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const Wino2Voxel v = wino2_voxel(a, h, m, wave, g, kh, z0, y0, x0);
        const bool in0 = whole || (v.gz < a.D && v.gy < a.H && v.gx < a.W), in1 = whole || (v.gz < a.D && v.gy + 1 < a.H && v.gx < a.W);
        float4 v0, v1;
        inverse_last(tq[h][0], tq[h][1], tq[h][2], tq[h][3], b4, v0, v1);
        if (bnr) {
            bn_bwd_reduce_pair(v0, v1, yv[h][0], yv[h][1], sc4, sh4, bm4, a.slope, s4, q4);     // (pulpo::bn_bwd_reduce_step, head_bn.h)
        } else if (whole) {
            stats_add_pair(v0, v1, s4, q4);
        } else {
            if (in0) stats_add_one(v0, s4, q4);
            if (in1) stats_add_one(v1, s4, q4);
        }
        if (fuse) {
            v0 = bn_lrelu4(v0, sc4, sh4, a.slope);
            v1 = bn_lrelu4(v1, sc4, sh4, a.slope);
        }
        if (in0) *reinterpret_cast<float4*>(obase + v.vox * o_ps) = v0;
        if (in1) *reinterpret_cast<float4*>(obase + (v.vox + a.W) * o_ps) = v1;
    }
}

}  // namespace pulpo_conv
