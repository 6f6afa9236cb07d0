// Mattes mutual information over a cubic-B-spline Parzen joint histogram.  No counterpart in the reference, whose
// losses all assume one contrast.
//
// mi_hist:   P = Wp^T Wt on the matrix cores (v_mfma_f32_32x32x2_f32, true fp32): the V x K weight matrices are formed in registers, two
//            voxels per MFMA, and never stored.  A wave keeps its K_pad x K_pad tile(s) in registers over all of its voxels; the four waves
//            of a workgroup are summed through LDS in wave order and the workgroup writes one slab row.  Dense, so its time does not
//            depend on the image content, and there is nothing to serialise on.
// mi_finish: one workgroup per batch element sums the slab rows in row order in double and forms p, MI_b and G = d MI_b / d P.
// mi_bwd:    a 4 x 4-tap gather from G (in LDS) per voxel.
// No atomics anywhere: bit-identical run to run.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxRows = 256;           // slab rows over the whole batch: 256 x 64 x 64 floats = 4 MiB at K > 32, 1 MiB at K <= 32
constexpr int kVoxPerBlock = 1024;      // a workgroup is worth starting for this many voxels (4 chunks of 64 per wave)
constexpr double kEps = 1e-12;

// slab rows (workgroups of mi_hist) per batch element: a function of the shape only
inline int rows_per_batch(int B, long V) { return (int)std::max<long>(1, std::min<long>((V + kVoxPerBlock - 1) / kVoxPerBlock, kMaxRows / B)); }

inline int kpad(int K) { return K <= 32 ? 32 : 64; }

// cubic B-spline and its derivative
__device__ __forceinline__ float beta3(float t) {
    const float a = fabsf(t), r = 2.f - a;
    const float inner = (2.f / 3.f) + a * a * (0.5f * a - 1.f);
    const float outer = r * r * r * (1.f / 6.f);
    return a < 1.f ? inner : (a < 2.f ? outer : 0.f);
}

__device__ __forceinline__ float dbeta3(float t) {
    const float a = fabsf(t), r = 2.f - a;
    const float inner = t * (1.5f * a - 2.f);
    const float outer = copysignf(0.5f * r * r, -t);
    return a < 1.f ? inner : (a < 2.f ? outer : 0.f);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// sum over a workgroup of 256 in a fixed order, valid in every thread (sh: 4 doubles of LDS); every thread must call it
__device__ __forceinline__ double block_sum_256_d(double v, double* sh) {
    v = pulpo::wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return t;
}

// grid (nb, B).  NT x NT accumulator tiles of 32 x 32 bins: pred's bin on the MFMA's row, true's on its column.  A wave loads 64 voxels, one
// per lane; step s of a chunk multiplies voxels s (lanes 0-31, k = 0) and s + 32 (lanes 32-63, k = 1), broadcast within each half-wave.
template <int NT>
__global__ __launch_bounds__(256) void mi_hist_kernel(const float* __restrict__ pred, const float* __restrict__ tru, const float* __restrict__ wa,
                                                        const float* __restrict__ wb, float* __restrict__ slab, long V, int K, int nb) {
    constexpr int KP = 32 * NT;
    __shared__ float red[KP * KP];
    const int b = blockIdx.y, j = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = lane & 31, half = lane & 32;
    const float sc = (float)(K - 3);
    pred += (long)b * V, tru += (long)b * V;
    if (wa != nullptr) wa += (long)b * V;
    if (wb != nullptr) wb += (long)b * V;
    f32x16 acc[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;
    const long nchunk = (V + 63) >> 6;
    for (long q = (long)j * 4 + wave; q < nchunk; q += (long)nb * 4) {
        const long v = q * 64 + lane;
        const long vl = v < V ? v : V - 1;            // the tail: a clamped load, zero weight
        float m = v < V ? 1.f : 0.f;
        if (wa != nullptr) {
            m *= wa[vl];
            if (wb != nullptr) m *= wb[vl];
        }
        const float up = clamp01(pred[vl]) * sc + 1.f, ut = clamp01(tru[vl]) * sc + 1.f;
#pragma unroll 4
        for (int s = 0; s < 32; ++s) {
            const int src = s + half;
            const float pu = __shfl(up, src, 64), tu = __shfl(ut, src, 64), mm = __shfl(m, src, 64);
            float av[NT], bv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                av[t] = mm * beta3(pu - (float)(bin + 32 * t));
                bv[t] = beta3(tu - (float)(bin + 32 * t));
            }
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
        }
    }
    // wave 0 stores, waves 1..3 add in turn: a fixed order
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        float* d = red + row * KP + 32 * tj + bin;
                        *d = w == 0 ? acc[ti][tj][r] : *d + acc[ti][tj][r];
                    }
        }
        __syncthreads();
    }
    float* out = slab + ((long)b * nb + j) * (KP * KP);
    for (int e = threadIdx.x; e < KP * KP; e += 256) out[e] = red[e];
}

// d MI / d p[a,c] of MI = sum p (log(p + e) - log(pa pb + e)), with R[a] = sum_c p[a,c] pb[c] / (pa[a] pb[c] + e) and C[c] likewise over a
__device__ __forceinline__ double mi_dp(double p, double q, double Ra, double Cc, double& term) {
    const double l = log(p + kEps) - log(q + kEps);
    term = p * l;
    return l + p / (p + kEps) - Ra - Cc;
}

// grid B, 256 threads, K * K doubles of dynamic LDS
__global__ __launch_bounds__(256) void mi_finish_kernel(const float* __restrict__ slab, int nb, int K, int KP, double* __restrict__ p_out,
                                                          double* __restrict__ mi_out, float* __restrict__ G_out) {
    extern __shared__ __align__(16) double pl[];
    __shared__ double pa[64], pb[64], R[64], Cc[64], sh[4];
    const int b = blockIdx.x, tid = threadIdx.x, KK = K * K;
    const float* rows = slab + (long)b * nb * (KP * KP);
    double local = 0.0;
    for (int e = tid; e < KK; e += 256) {
        const int a = e / K, c = e - a * K;
        double s = 0.0;
        for (int r = 0; r < nb; ++r) s += (double)rows[(long)r * (KP * KP) + a * KP + c];
        pl[e] = s;
        local += s;
    }
    const double M = block_sum_256_d(local, sh);         // = sum of the voxel weights: every voxel's weights sum to 1
    double* po = p_out + (long)b * KK;
    float* Go = G_out + (long)b * KK;
    if (!(M > 0.0)) {                                     // an empty mask: MI 0, no gradient
        for (int e = tid; e < KK; e += 256) po[e] = 0.0, Go[e] = 0.f;
        if (tid == 0) mi_out[b] = 0.0;
        return;
    }
    for (int e = tid; e < KK; e += 256) pl[e] /= M;
    __syncthreads();
    if (tid < K) {
        double s = 0.0;
        for (int c = 0; c < K; ++c) s += pl[tid * K + c];
        pa[tid] = s;
    } else if (tid >= 64 && tid < 64 + K) {
        const int c = tid - 64;
        double s = 0.0;
        for (int a = 0; a < K; ++a) s += pl[a * K + c];
        pb[c] = s;
    }
    __syncthreads();
    if (tid < K) {
        double s = 0.0;
        for (int c = 0; c < K; ++c) s += pl[tid * K + c] * pb[c] / (pa[tid] * pb[c] + kEps);
        R[tid] = s;
    } else if (tid >= 64 && tid < 64 + K) {
        const int c = tid - 64;
        double s = 0.0;
        for (int a = 0; a < K; ++a) s += pl[a * K + c] * pa[a] / (pa[a] * pb[c] + kEps);
        Cc[c] = s;
    }
    __syncthreads();
    double mi = 0.0, pg = 0.0;
    for (int e = tid; e < KK; e += 256) {
        const int a = e / K, c = e - a * K;
        double term;
        const double g = mi_dp(pl[e], pa[a] * pb[c], R[a], Cc[c], term);
        mi += term;
        pg += pl[e] * g;
    }
    const double MI = block_sum_256_d(mi, sh);
    const double S = block_sum_256_d(pg, sh);
    for (int e = tid; e < KK; e += 256) {               // d p[a,c] / d P[i,j] = (delta - p[a,c]) / M
        const int a = e / K, c = e - a * K;
        double term;
        const double g = mi_dp(pl[e], pa[a] * pb[c], R[a], Cc[c], term);
        po[e] = pl[e];
        Go[e] = (float)((g - S) / M);
    }
    if (tid == 0) mi_out[b] = MI;
}

// loss = -gamma V mean_b MI_b, the batch summed in order
__global__ void mi_loss_kernel(const double* __restrict__ mi, int B, double scale, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += mi[b];
    loss[0] = (float)(scale * s);
}

// d (sum_ac G[a,c] P[a,c]) / d pred_v over m_v (K - 3): the 4 x 4 taps around (u(pred_v), u(true_v)).  u is in [1, K - 2], so the first tap is
// bin floor(u) - 1 >= 0; the last can be bin K, where both beta3 and its derivative are 0 - its index is clamped, its weight is not.
__device__ __forceinline__ float mi_grad_voxel(const float* __restrict__ g, float pv, float tv, int K, float sc) {
    if (!(pv >= 0.f && pv <= 1.f)) return 0.f;          // torch.clamp's gradient: passes on [0,1], ends included
    const float up = pv * sc + 1.f, ut = clamp01(tv) * sc + 1.f;
    const int ia = (int)floorf(up) - 1, ic = (int)floorf(ut) - 1;
    float wc[4];
    int jc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        wc[s] = beta3(ut - (float)(ic + s));
        jc[s] = min(ic + s, K - 1);
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float* row = g + min(ia + t, K - 1) * K;
        const float inner = ((wc[0] * row[jc[0]] + wc[1] * row[jc[1]]) + wc[2] * row[jc[2]]) + wc[3] * row[jc[3]];
        sum += dbeta3(up - (float)(ia + t)) * inner;
    }
    return sum;
}

// grid (blocks, B), K * K floats of dynamic LDS.  VEC 4: V % 4 == 0 and 16-byte aligned planes
template <int VEC>
__global__ __launch_bounds__(256) void mi_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tru, const float* __restrict__ wa,
                                                       const float* __restrict__ wb, const float* __restrict__ G, const float* __restrict__ gscale,
                                                       float coef, float* __restrict__ gpred, long V, int K) {
    extern __shared__ __align__(16) float g[];
    const int b = blockIdx.y;
    for (int e = threadIdx.x; e < K * K; e += 256) g[e] = G[(long)b * K * K + e];
    __syncthreads();
    const float sc = (float)(K - 3);
    const float k0 = coef * (gscale != nullptr ? gscale[0] : 1.f) * sc;
    const long off = (long)b * V;
    pred += off, tru += off, gpred += off;
    if (wa != nullptr) wa += off;
    if (wb != nullptr) wb += off;
    const long n = V / VEC;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        if constexpr (VEC == 4) {
            const float4 p4 = reinterpret_cast<const float4*>(pred)[i], t4 = reinterpret_cast<const float4*>(tru)[i];
            float4 m4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if (wa != nullptr) {
                m4 = reinterpret_cast<const float4*>(wa)[i];
                if (wb != nullptr) {
                    const float4 n4 = reinterpret_cast<const float4*>(wb)[i];
                    m4.x *= n4.x, m4.y *= n4.y, m4.z *= n4.z, m4.w *= n4.w;
                }
            }
            float4 o;
            o.x = k0 * m4.x * mi_grad_voxel(g, p4.x, t4.x, K, sc);
            o.y = k0 * m4.y * mi_grad_voxel(g, p4.y, t4.y, K, sc);
            o.z = k0 * m4.z * mi_grad_voxel(g, p4.z, t4.z, K, sc);
            o.w = k0 * m4.w * mi_grad_voxel(g, p4.w, t4.w, K, sc);
            reinterpret_cast<float4*>(gpred)[i] = o;
        } else {
            float m = 1.f;
            if (wa != nullptr) {
                m = wa[i];
                if (wb != nullptr) m *= wb[i];
            }
            gpred[i] = k0 * m * mi_grad_voxel(g, pred[i], tru[i], K, sc);
        }
    }
}

static int check_args(const char* who, int B, int64_t V, int K) {
    PULPO_REQUIRE(B >= 1 && V >= 1, "%s: B and V must be >= 1 (got B %d, V %lld)", who, B, (long long)V);
    PULPO_REQUIRE(B <= 65535, "%s: at most 65535 batch elements (got %d)", who, B);
    PULPO_REQUIRE(V < (1LL << 40), "%s: at most 2^40 voxels per batch element", who);
    PULPO_REQUIRE(K >= 4 && K <= 64, "%s: bins must be in [4, 64] (got %d)", who, K);
    return 0;
}

static bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

}  // namespace

// slab rows of pulpo_mi_fwd (= workgroups of the histogram kernel) over the whole batch; 0 for arguments the entry points refuse
PULPO_API int pulpo_mi_blocks(int B, int64_t V) {
    if (B < 1 || B > 65535 || V < 1) return 0;
    return B * rows_per_batch(B, (long)V);
}

// floats of pulpo_mi_fwd's scratch (the slab); 0 for arguments the entry points refuse
PULPO_API int64_t pulpo_mi_scratch_floats(int B, int64_t V, int K) {
    if (B < 1 || B > 65535 || V < 1 || K < 4 || K > 64) return 0;
    return (int64_t)B * rows_per_batch(B, (long)V) * kpad(K) * kpad(K);
}

PULPO_API int pulpo_mi_fwd(const float* y_true, const float* y_pred, const float* wa, const float* wb, float* scratch, double* p, double* mi, float* G,
                           float* loss, int B, int64_t V, int K, double gamma, void* stream) {
    PULPO_REQUIRE(y_true && y_pred && scratch && p && mi && G && loss && (wa || !wb), "mi_fwd: bad arguments");
    if (int rc = check_args("mi_fwd", B, V, K)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nb = rows_per_batch(B, (long)V), KP = kpad(K);
    if (KP == 32) hipLaunchKernelGGL(mi_hist_kernel<1>, dim3(nb, B), dim3(256), 0, st, y_pred, y_true, wa, wb, scratch, (long)V, K, nb);
    else hipLaunchKernelGGL(mi_hist_kernel<2>, dim3(nb, B), dim3(256), 0, st, y_pred, y_true, wa, wb, scratch, (long)V, K, nb);
    if (int rc = pulpo::check_launch("mi_fwd hist")) return rc;
    hipLaunchKernelGGL(mi_finish_kernel, dim3(B), dim3(256), (size_t)K * K * sizeof(double), st, scratch, nb, K, KP, p, mi, G);
    if (int rc = pulpo::check_launch("mi_fwd finish")) return rc;
    hipLaunchKernelGGL(mi_loss_kernel, dim3(1), dim3(64), 0, st, mi, B, -gamma * (double)V / (double)B, loss);
    return pulpo::check_launch("mi_fwd loss");
}

PULPO_API int pulpo_mi_bwd(const float* y_true, const float* y_pred, const float* wa, const float* wb, const float* G, const float* gscale, float coef,
                           float* gpred, int B, int64_t V, int K, void* stream) {
    PULPO_REQUIRE(y_true && y_pred && G && gpred && (wa || !wb), "mi_bwd: bad arguments");
    if (int rc = check_args("mi_bwd", B, V, K)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)K * K * sizeof(float);
    const bool vec = V % 4 == 0 && aligned16(y_true) && aligned16(y_pred) && aligned16(wa) && aligned16(wb) && aligned16(gpred);
    const int grid = pulpo::eblocks(vec ? V / 4 : V, std::max(1, 2048 / B));
    if (vec) hipLaunchKernelGGL(mi_bwd_kernel<4>, dim3(grid, B), dim3(256), lds, st, y_pred, y_true, wa, wb, G, gscale, coef, gpred, (long)V, K);
    else hipLaunchKernelGGL(mi_bwd_kernel<1>, dim3(grid, B), dim3(256), lds, st, y_pred, y_true, wa, wb, G, gscale, coef, gpred, (long)V, K);
    return pulpo::check_launch("mi_bwd");
}
