// Inverse deformation fields (inference only: no backward kernels; the paired integration that keeps its intermediate fields for a
// backward pass, and that pass, sit beside the step kernels they reuse, in warp.hip: pulpo_vecint_pair_fwd_work / pulpo_vecint_pair_bwd).
//   pulpo_vecint_pair_fwd       fwd = VecInt(v) and inv = VecInt(-v) in one call (network_blocks.py:160-177 run on v and on -v): the level
//                               fields are stationary velocity fields, so the inverse of the flow is the integral of the negated velocity.
//                               Coordinates are pulpo::sample_coord's, the step is pulpo::vecint_step_voxel: fwd is pulpo_vecint_fwd's result.
//                               No intermediate field is kept (pulpo_vecint_fwd stores nsteps + 1 of them for a backward pass).
//   pulpo_inverse_consistency   mean and maximum over the voxels of ||b(p) + a(p + b(p))||_2, the distance of a o b from the identity.
//   pulpo_transport_points      out = pts + field(pts): points carried by a field sampled at their own (fractional) positions; with the
//                               inverse field this is the exact form of the landmark rule of evaluate.py:410-423, long(lm) - df[long(lm)],
//                               which is its first-order approximation evaluated at a truncated position.
// The last two use the GEOMETRIC composition (pulpo::geo_coord): positions in voxel units clamped to [0, S - 1], trilinear with upper
// corner min(i0 + 1, S - 1).  That is deliberately not the reference SpatialTransformer's (S-1)-normalised, align_corners=False sampling,
// whose zero field is not the identity: it treats a field the way the reference's landmark rule does, as displacements
// in voxels at voxel centres.
#include "common.h"
#include "sampling.h"

namespace {

using pulpo::GeoCorner;
using pulpo::geo_coord;
using pulpo::geo_sample;

// fields of up to this many voxels per batch element take the one-launch form (the switch of pulpo_vecint_fwd)
constexpr int PAIR_LDS_MAXV = 2048, PAIR_THREADS = 1024, PAIR_VPT = PAIR_LDS_MAXV / PAIR_THREADS;

// All squaring steps in one launch with the field in LDS, as vecint_fwd_lds_kernel does; one workgroup per (batch element, direction):
// block 2 b integrates +v into fwd[b], block 2 b + 1 integrates -v into inv[b].  Only the last field leaves the workgroup.
__global__ __launch_bounds__(PAIR_THREADS) void vecint_pair_lds_kernel(const float* __restrict__ v, float* __restrict__ fwd, float* __restrict__ inv,
                                                                        int D, int H, int W, int nsteps, float scale) {
    __shared__ float fld[3 * PAIR_LDS_MAXV];           // [3][V]
    const int V = D * H * W, tid = threadIdx.x;
    const long b = blockIdx.x >> 1;
    const bool neg = blockIdx.x & 1;
    const float sc = neg ? -scale : scale;
    for (int i = tid; i < 3 * V; i += PAIR_THREADS) fld[i] = v[b * 3 * V + i] * sc;
    __syncthreads();
    for (int k = 0; k < nsteps; ++k) {
        float nv[PAIR_VPT][3];
#pragma unroll
        for (int j = 0; j < PAIR_VPT; ++j) {
            const int vox = tid + j * PAIR_THREADS;
            if (vox < V) pulpo::vecint_step_voxel(fld, V, vox, D, H, W, nv[j]);
        }
        __syncthreads();                               // every gather of this step is done: the field may be overwritten
#pragma unroll
        for (int j = 0; j < PAIR_VPT; ++j) {
            const int vox = tid + j * PAIR_THREADS;
            if (vox < V) {
#pragma unroll
                for (int c = 0; c < 3; ++c) fld[c * V + vox] = nv[j][c];
            }
        }
        __syncthreads();
    }
    float* out = (neg ? inv : fwd) + b * 3 * V;
    for (int i = tid; i < 3 * V; i += PAIR_THREADS) out[i] = fld[i];
}

// pos = v * scale, neg = -v * scale (scale = 2^-nsteps: both exact)
__global__ __launch_bounds__(256) void pair_scale_kernel(const float* __restrict__ v, float* __restrict__ pos, float* __restrict__ neg, float scale, long n) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const float val = v[e] * scale;
        pos[e] = val;
        neg[e] = -val;
    }
}

// One squaring step of both directions: items [0, B V) advance src0 -> dst0, items [B V, 2 B V) advance src1 -> dst1.
__global__ __launch_bounds__(256) void vecint_pair_step_kernel(const float* __restrict__ src0, const float* __restrict__ src1, float* __restrict__ dst0,
                                                                float* __restrict__ dst1, int B, int D, int H, int W) {
    const int V = D * H * W;
    const long BV = (long)B * V;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < 2 * BV; e += (long)gridDim.x * blockDim.x) {
        const bool second = e >= BV;
        const long r = second ? e - BV : e;
        const long b = B == 1 ? 0 : r / V;               // (one 64-bit division per voxel at most, as in warp_fwd_kernel)
        const int vox = (int)(r - b * V);
        const float* s = (second ? src1 : src0) + b * 3 * V;
        float* d = (second ? dst1 : dst0) + b * 3 * V;
        float nv[3];
        pulpo::vecint_step_voxel(s, V, vox, D, H, W, nv);
        d[vox] = nv[0];
        d[(long)V + vox] = nv[1];
        d[2 * (long)V + vox] = nv[2];
    }
}

using pulpo::eblocks;

inline bool pair_lds(int D, int H, int W, int nsteps) { return nsteps > 0 && (long)D * H * W <= PAIR_LDS_MAXV; }

// Per voxel p (one thread, lanes along x): r = b(p) + a(p + b(p)) with the geometric sampler, in double; per thread the sum and the
// maximum of ||r||; per block one partial of each, in double.  nd = 2 (D == 1, two-channel fields) or 3.
__global__ __launch_bounds__(256) void inverse_consistency_kernel(const float* __restrict__ a, const float* __restrict__ bf, int B, int D, int H, int W,
                                                                   int nd, double* __restrict__ psum, double* __restrict__ pmax) {
    __shared__ double shs[4], shm[4];
    const int V = D * H * W;
    const long total = (long)B * V;
    double s = 0.0, m = 0.0;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long b = B == 1 ? 0 : e / V;
        const int vox = (int)(e - b * V);
        const int x = vox % W, y = (vox / W) % H, z = vox / (W * H);
        const float* bp = bf + b * nd * V + vox;
        const float* ap = a + b * nd * V;
        double bz = 0.0, by, bx;
        if (nd == 3) { bz = bp[0]; by = bp[V]; bx = bp[2 * (long)V]; }
        else { by = bp[0]; bx = bp[V]; }
        const GeoCorner cz = geo_coord((double)z + bz, D), cy = geo_coord((double)y + by, H), cx = geo_coord((double)x + bx, W);
        double q = 0.0;
        if (nd == 3) {
            const double rz = bz + geo_sample(ap, cz, cy, cx, H, W);
            q = rz * rz;
            ap += V;
        }
        const double ry = by + geo_sample(ap, cz, cy, cx, H, W), rx = bx + geo_sample(ap + V, cz, cy, cx, H, W);
        q += ry * ry + rx * rx;
        const double nrm = sqrt(q);
        s += nrm;
        m = fmax(m, nrm);
    }
    s = pulpo::wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) {
        shs[threadIdx.x >> 6] = s;
        shm[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = (shs[0] + shs[1]) + (shs[2] + shs[3]);
        pmax[blockIdx.x] = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
    }
}

// one wave: lane t adds partials t, t + 64, ... in that order, then the butterfly - the same order on every call.  out = (mean, max)
__global__ void inverse_consistency_finalize_kernel(const double* __restrict__ psum, const double* __restrict__ pmax, int nblk, double n,
                                                    float* __restrict__ out) {
    double s = 0.0, m = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) { s += psum[k]; m = fmax(m, pmax[k]); }
    s = pulpo::wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) {
        out[0] = (float)(s / n);
        out[1] = (float)m;
    }
}

inline int consistency_blocks(int B, int D, int H, int W) { return eblocks((long)B * D * H * W, 1024); }

// out[s][k][c] = pts[k][c] + trilinear(field[s][c], clamp(pts[k])); flag[0] = 1 if a point lies outside [0, S - 1] (or is not a number)
__global__ void transport_points_kernel(const float* __restrict__ pts, const float* __restrict__ field, float* __restrict__ out, int npts, int nsamp,
                                        int nd, int D, int H, int W, int* __restrict__ flag) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)npts * nsamp) return;
    const int k = (int)(t % npts);
    const long s = t / npts;
    const int S[3] = {D, H, W};
    double p[3] = {0.0, 0.0, 0.0};                      // (z, y, x); 2-D points are (y, x) on a depth-1 field
    bool ok = true;
    for (int c = 0; c < nd; ++c) {
        const int dim = nd == 3 ? c : c + 1;
        const double val = pts[(long)k * nd + c];
        p[dim] = val;
        ok = ok && val >= 0.0 && val <= (double)(S[dim] - 1);
    }
    if (!ok) atomicOr(flag, 1);
    const GeoCorner cz = geo_coord(p[0], D), cy = geo_coord(p[1], H), cx = geo_coord(p[2], W);
    const long V = (long)D * H * W;
    for (int c = 0; c < nd; ++c) {
        const int dim = nd == 3 ? c : c + 1;
        out[(s * npts + k) * nd + c] = (float)(p[dim] + geo_sample(field + (s * nd + c) * V, cz, cy, cx, H, W));
    }
}

}  // namespace

// floats of scratch pulpo_vecint_pair_fwd needs: two fields for the step form, none for the one-launch form and for nsteps == 0
PULPO_API size_t pulpo_vecint_pair_scratch_floats(int B, int D, int H, int W, int nsteps) {
    if (B <= 0 || D < 1 || H < 1 || W < 1 || nsteps <= 0 || pair_lds(D, H, W, nsteps)) return 0;
    return 2 * (size_t)B * 3 * D * H * W;
}

// v, fwd, inv: (B,3,D,H,W) planar (D == 1: the 2-D form, channel 0 zero).  scratch: pulpo_vecint_pair_scratch_floats() floats (NULL when 0).
PULPO_API int pulpo_vecint_pair_fwd(const float* v, float* fwd, float* inv, float* scratch, int B, int D, int H, int W, int nsteps, void* stream) {
    PULPO_REQUIRE(v && fwd && inv && B > 0 && D >= 1 && H > 1 && W > 1 && nsteps >= 0 && nsteps < 31 && (long)D * H * W < (1L << 31),
                  "vecint_pair_fwd: bad arguments");
    PULPO_REQUIRE(scratch || pulpo_vecint_pair_scratch_floats(B, D, H, W, nsteps) == 0,
                  "vecint_pair_fwd: scratch of pulpo_vecint_pair_scratch_floats() floats required");
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)B * 3 * D * H * W, total = (long)B * D * H * W;
    const float scale = 1.0f / (float)(1 << nsteps);
    if (pair_lds(D, H, W, nsteps)) {
        hipLaunchKernelGGL(vecint_pair_lds_kernel, dim3(2 * B), dim3(PAIR_THREADS), 0, st, v, fwd, inv, D, H, W, nsteps, scale);
        return pulpo::check_launch("vecint_pair_lds");
    }
    // ping-pong between (fwd, inv) and the two scratch fields: the field after k squarings sits in the outputs when nsteps - k is even,
    // so the last step lands in fwd / inv whatever the parity of nsteps
    float* bufs[2][2] = {{fwd, inv}, {scratch, scratch ? scratch + n : nullptr}};
    int side = nsteps & 1;
    hipLaunchKernelGGL(pair_scale_kernel, dim3(eblocks(n, 8192)), dim3(256), 0, st, v, bufs[side][0], bufs[side][1], scale, n);
    int rc = pulpo::check_launch("vecint_pair scale");
    if (rc) return rc;
    for (int k = 0; k < nsteps; ++k, side ^= 1) {
        hipLaunchKernelGGL(vecint_pair_step_kernel, dim3(eblocks(2 * total, 8192)), dim3(256), 0, st, bufs[side][0], bufs[side][1], bufs[side ^ 1][0],
                           bufs[side ^ 1][1], B, D, H, W);
        rc = pulpo::check_launch("vecint_pair step");
        if (rc) return rc;
    }
    return 0;
}

PULPO_API size_t pulpo_inverse_consistency_ws_bytes(int B, int D, int H, int W) {
    if (B <= 0 || D < 1 || H < 1 || W < 1) return 0;
    return (size_t)consistency_blocks(B, D, H, W) * 2 * sizeof(double);
}

// a, b: (B,3,D,H,W) planar, or (B,2,1,H,W) when D == 1.  out: 2 floats (mean, max of ||b(p) + a(p + b(p))||).  ws: the query's bytes.
PULPO_API int pulpo_inverse_consistency(const float* a, const float* b, float* out, void* ws, int B, int D, int H, int W, void* stream) {
    PULPO_REQUIRE(a && b && out && ws && B > 0 && D >= 1 && H > 0 && W > 0 && (long)D * H * W < (1L << 31), "inverse_consistency: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = consistency_blocks(B, D, H, W);
    double* psum = (double*)ws;
    double* pmax = psum + nblk;
    hipLaunchKernelGGL(inverse_consistency_kernel, dim3(nblk), dim3(256), 0, st, a, b, B, D, H, W, D == 1 ? 2 : 3, psum, pmax);
    int rc = pulpo::check_launch("inverse_consistency");
    if (rc) return rc;
    hipLaunchKernelGGL(inverse_consistency_finalize_kernel, dim3(1), dim3(64), 0, st, psum, pmax, nblk, (double)B * D * H * W, out);
    return pulpo::check_launch("inverse_consistency finalize");
}

// pts: (npts, nd) voxel coordinates; field: (nsamp, nd, D, H, W) planar (nd == 2: D must be 1); out: (nsamp, npts, nd);
// flag: one int, zeroed here, set to 1 when a point lies outside the field
PULPO_API int pulpo_transport_points(const float* pts, const float* field, float* out, int npts, int nsamp, int nd, int D, int H, int W, int* flag,
                                     void* stream) {
    PULPO_REQUIRE(pts && field && out && flag && npts > 0 && nsamp > 0 && (nd == 3 || (nd == 2 && D == 1)) && D > 0 && H > 0 && W > 0,
                  "transport_points: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e != hipSuccess) return pulpo::fail((int)e, "transport_points memset: %s", hipGetErrorString(e));
    const long n = (long)npts * nsamp;
    hipLaunchKernelGGL(transport_points_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, pts, field, out, npts, nsamp, nd, D, H, W, flag);
    return pulpo::check_launch("transport_points");
}
