// Boundary metrics of a registration: the exact squared Euclidean distance transform of a voxel set and, built on
// it, the Hausdorff distance, its percentile form (HD95) and the average symmetric surface distance between the class surfaces of two
// label maps.  Pure integer arithmetic up to the final square roots: results are exact and bit-identical from run to run.
//
// The transform is separable.  Row pass (along W): one wave per row; the row's feature bits are gathered with one ballot per 64 voxels
// (<= 16 words for a row of 1024), and every voxel finds its nearest feature to the left and to the right by counting leading / trailing
// zeros in those words.  Line passes (along H, then along D): out(i) = min_j g(j) + (i - j)^2.  A workgroup holds a tile of one whole line
// x XT consecutive x in LDS (XT = 64 for lines up to 240, 32 up to 480, 16 up to 960, 8 beyond: at most 60 KB), so that global reads and writes
// run along W, and takes the minimum over the line by brute force: lanes read consecutive x of one j (no bank conflict), and every value
// read serves four outputs of the thread.  The tile is loaded whole before anything is written and no other workgroup touches it, so the
// line passes run in place.  In-pass infinity is 1 << 29 (+ 1023^2 stays in int32) and every pass clamps to it: an empty set gives the
// constant EDT_INF.
//
// Surface distances: the features of the row pass are the surface voxels of class c in one label map, tested on the label map itself
// (a voxel of the class with a face neighbour outside it, the volume's outside included; no mask or one-hot tensor exists); the last line
// pass is evaluated only at the surface voxels of class c in the other map, each of which adds 1 to an integer histogram over d^2
// (bins below 64 first collect in LDS: near-aligned surfaces put most voxels there).  A finalize kernel turns the two histograms of a class
// into HD, HDq, ASSD in double.  Classes are processed in chunks of a size fixed by B and the volume, not by C.
#include "common.h"

#include <type_traits>

namespace {

constexpr int kInf = 1 << 29;
constexpr int kMaxExtent = 1024;
constexpr int kNoFeature = 1 << 20;          // a 1-D distance no row reaches
constexpr int kLdsBins = 64;
constexpr size_t kChunkBytes = (size_t)1 << 26;

template <typename LT>
__device__ __forceinline__ bool is_surface(const LT* __restrict__ lab, int c, int z, int y, int x, int D, int H, int W, int nd) {
    const long i = ((long)z * H + y) * W + x;
    if ((int)lab[i] != c) return false;
    bool s = x == 0 || (int)lab[i - 1] != c;
    s |= x == W - 1 || (int)lab[i + 1] != c;
    s |= y == 0 || (int)lab[i - W] != c;
    s |= y == H - 1 || (int)lab[i + W] != c;
    if (nd == 3) {
        const long hw = (long)H * W;
        s |= z == 0 || (int)lab[i - hw] != c;
        s |= z == D - 1 || (int)lab[i + hw] != c;
    }
    return s;
}

// Row pass.  One wave per row, four rows per workgroup; rows = planes * D * H.  LT = void: the features are the non-zero bytes of `src`
// (planes = B); otherwise the surface voxels of class c0 + plane % CH of the label map `src` (planes = B * CH, item = plane / CH), whose
// labels are range-checked into *flag on the way.
template <typename LT>
__global__ __launch_bounds__(256) void row_pass_kernel(const void* __restrict__ src, int* __restrict__ g, long rows, int D, int H, int W, int nd, int CH,
                                                         int c0, int C, int* __restrict__ flag) {
    __shared__ unsigned long long words[4][kMaxExtent / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wv;
    const bool live = row < rows;
    const int nw = (W + 63) >> 6;
    const long dh = (long)D * H;
    const long plane = live ? row / dh : 0;
    const int rem = live ? (int)(row - plane * dh) : 0;
    const int z = rem / H, y = rem - z * H;
    const long V = dh * W;
    int item = (int)plane, c = 0;
    if constexpr (!std::is_void<LT>::value) {
        item = (int)(plane / CH);
        c = c0 + (int)(plane - (long)item * CH);
    }
    bool bad = false;
    for (int s = 0; s < nw; ++s) {
        const int x = s * 64 + lane;
        bool f = false;
        if (live && x < W) {
            if constexpr (std::is_void<LT>::value) {
                f = ((const uint8_t*)src)[(long)item * V + ((long)z * H + y) * W + x] != 0;
            } else {
                const LT* lab = (const LT*)src + (long)item * V;
                const int l = (int)lab[((long)z * H + y) * W + x];
                bad |= l < 0 || l >= C;
                f = is_surface(lab, c, z, y, x, D, H, W, nd);
            }
        }
        const unsigned long long wd = __ballot(f);
        if (lane == 0) words[wv][s] = wd;
    }
    __syncthreads();
    if (!live) return;
    if constexpr (!std::is_void<LT>::value) {
        if (bad) atomicOr(flag, 1);
    }
    int* out = g + plane * V + ((long)z * H + y) * W;
    for (int s = 0; s < nw; ++s) {
        const int x = s * 64 + lane;
        int left = -1, right = -1;
        for (int k = 0; k < nw; ++k) {
            const unsigned long long wk = words[wv][k];
            if (k < s) {
                if (wk) left = k * 64 + 63 - __clzll((long long)wk);
            } else if (k == s) {
                const unsigned long long lo = wk & (~0ull >> (63 - lane)), hi = wk & (~0ull << lane);
                if (lo) left = k * 64 + 63 - __clzll((long long)lo);
                if (hi) right = k * 64 + __ffsll((long long)hi) - 1;
            } else if (right < 0 && wk) {
                right = k * 64 + __ffsll((long long)wk) - 1;
            }
        }
        const int dl = left >= 0 ? x - left : kNoFeature, dr = right >= 0 ? right - x : kNoFeature;
        const int d = dl < dr ? dl : dr;
        if (x < W) out[x] = d >= kNoFeature ? kInf : d * d;
    }
}

// Line pass over lines of n entries `lstride` apart.  grid (x tiles, lines' other axis, planes); the tile's first element is
// plane * V + blockIdx.y * ostride + blockIdx.x * XT.  XT = 1 << xshift.  LT = void: every output is written back in place.  Otherwise (the
// last pass, lines along D, blockIdx.y = y): an output is formed only at the surface voxels of class c of `lab`, and counted in
// hist[((item * C + c) * 2 + which) * bins + d^2] - an output of kInf (no feature in the other map) is left out - and the number of such
// voxels is added to cnt[(item * C + c) * 2 + which] (one global add per workgroup).
template <typename LT>
__global__ __launch_bounds__(256) void line_pass_kernel(int* __restrict__ g, int n, long lstride, long ostride, int W, int xshift, long V,
                                                          const LT* __restrict__ lab, int D, int H, int nd, int CH, int c0, int C, int which,
                                                          int* __restrict__ hist, int bins, int* __restrict__ cnt) {
    extern __shared__ int tile[];
    __shared__ int lh[kLdsBins + 1];          // the last entry counts the workgroup's evaluated voxels
    const int XT = 1 << xshift;
    const int x0 = blockIdx.x << xshift;
    const long plane = blockIdx.z;
    int* base = g + plane * V + (long)blockIdx.y * ostride + x0;
    for (int e = threadIdx.x; e < (n << xshift); e += 256) {
        const int j = e >> xshift, xx = e & (XT - 1);
        tile[e] = x0 + xx < W ? base[(long)j * lstride + xx] : kInf;
    }
    constexpr bool kHist = !std::is_void<LT>::value;
    if (kHist && threadIdx.x <= kLdsBins) lh[threadIdx.x] = 0;
    __syncthreads();
    const int xi = threadIdx.x & (XT - 1), grp = threadIdx.x >> xshift, G = 256 >> xshift;
    const int x = x0 + xi;
    int item = 0, c = 0;
    if constexpr (kHist) {
        item = (int)(plane / CH);
        c = c0 + (int)(plane - (long)item * CH);
    }
    int evaluated = 0;
    if (x < W) {
        for (int ib = grp; ib < n; ib += 4 * G) {
            int i[4], r[4];
            bool want[4];
            bool any = false;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                i[m] = ib + m * G;
                r[m] = kInf;
                want[m] = i[m] < n;
                if constexpr (kHist) want[m] = want[m] && is_surface(lab + (long)item * V, c, i[m], (int)blockIdx.y, x, D, H, W, nd);
                any |= want[m];
            }
            if (!any) continue;
            for (int j = 0; j < n; ++j) {
                const int v = tile[(j << xshift) + xi];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int d = j - i[m];
                    const int cand = v + __mul24(d, d);
                    r[m] = cand < r[m] ? cand : r[m];
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!want[m]) continue;
                if constexpr (kHist) {
                    ++evaluated;
                    if (r[m] < kLdsBins) atomicAdd(&lh[r[m]], 1);
                    else if (r[m] < bins) atomicAdd(&hist[(((long)item * C + c) * 2 + which) * bins + r[m]], 1);
                } else {
                    base[(long)i[m] * lstride + xi] = r[m];
                }
            }
        }
    }
    if constexpr (kHist) {
        if (evaluated) atomicAdd(&lh[kLdsBins], evaluated);
        __syncthreads();
        if (threadIdx.x < kLdsBins && threadIdx.x < bins && lh[threadIdx.x])
            atomicAdd(&hist[(((long)item * C + c) * 2 + which) * bins + threadIdx.x], lh[threadIdx.x]);
        if (threadIdx.x == kLdsBins && lh[kLdsBins]) atomicAdd(&cnt[((long)item * C + c) * 2 + which], lh[kLdsBins]);
    }
}

// One workgroup per (item, class): out[5] = HD, HDq, ASSD, n_a, n_b from the class's two histograms.  Thread t owns a contiguous run of
// bins; the 256 run totals are scanned and summed by thread 0 in run order, so the double sums have one fixed order.
__global__ __launch_bounds__(256) void surface_finalize_kernel(const int* __restrict__ hist, const int* __restrict__ cnt, int bins, double q,
                                                                 float* __restrict__ out) {
    __shared__ long long s_cnt[256];
    __shared__ double s_sum[256];
    __shared__ int s_max[256];
    __shared__ int s_k[2];
    __shared__ double s_res[2][3];        // per direction: max d, percentile, sum d
    const int bc = blockIdx.x, t = threadIdx.x;
    const int n_a = cnt[2 * bc], n_b = cnt[2 * bc + 1];
    float* o = out + 5L * bc;
    if (n_a == 0 || n_b == 0) {
        if (t == 0) {
            const float nan = __int_as_float(0x7fc00000);
            o[0] = nan; o[1] = nan; o[2] = nan; o[3] = (float)n_a; o[4] = (float)n_b;
        }
        return;
    }
    if (t < 2) s_k[t] = 0;
    const int run = (bins + 255) / 256;
    const int lo = min(t * run, bins), hi = min(lo + run, bins);
    for (int dir = 0; dir < 2; ++dir) {
        const int* h = hist + ((long)bc * 2 + dir) * bins;
        const long long n = dir == 0 ? n_a : n_b;
        long long cs = 0;
        double ss = 0.0;
        int mx = 0;
        for (int k = lo; k < hi; ++k) {
            const int v = h[k];
            if (v) { cs += v; ss += sqrt((double)k) * (double)v; mx = k; }
        }
        s_cnt[t] = cs; s_sum[t] = ss; s_max[t] = mx;
        __syncthreads();
        if (t == 0) {
            long long off = 0;
            double tot = 0.0;
            int m = 0;
            for (int u = 0; u < 256; ++u) {
                const long long cu = s_cnt[u];
                s_cnt[u] = off;                       // exclusive offsets
                off += cu;
                tot += s_sum[u];
                m = s_max[u] > m ? s_max[u] : m;
            }
            s_res[dir][0] = sqrt((double)m);
            s_res[dir][2] = tot;
        }
        __syncthreads();
        // order statistics i0 = floor(rank), i1 = i0 + 1 (clamped): the thread whose run holds the index walks to it
        const double rank = q / 100.0 * (double)(n - 1);
        const long long i0 = (long long)floor(rank), i1 = i0 + 1 < n ? i0 + 1 : n - 1;
        const long long mine = s_cnt[t];
        for (int w = 0; w < 2; ++w) {
            const long long idx = w == 0 ? i0 : i1;
            if (cs > 0 && idx >= mine && idx < mine + cs) {
                long long acc = mine;
                for (int k = lo; k < hi; ++k) {
                    acc += h[k];
                    if (idx < acc) { s_k[w] = k; break; }
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            const double a = sqrt((double)s_k[0]), b = sqrt((double)s_k[1]), fr = rank - (double)i0;
            s_res[dir][1] = fr >= 0.5 ? b - (b - a) * (1.0 - fr) : a + (b - a) * fr;       // numpy's lerp
        }
        __syncthreads();
    }
    if (t == 0) {
        o[0] = (float)fmax(s_res[0][0], s_res[1][0]);
        o[1] = (float)fmax(s_res[0][1], s_res[1][1]);
        o[2] = (float)((s_res[0][2] + s_res[1][2]) / (double)((long long)n_a + n_b));
        o[3] = (float)n_a;
        o[4] = (float)n_b;
    }
}

// x extent of a line pass's tile: the widest power of two <= 64 at which line x tile stays within kTileInts of LDS (60 KB)
constexpr int kTileInts = 15360;
inline int tile_shift(int n) {
    int s = 6;
    while ((n << s) > kTileInts) --s;
    return s;
}

inline bool extents_ok(int B, int D, int H, int W) {
    return B > 0 && D >= 1 && H >= 1 && W >= 1 && D <= kMaxExtent && H <= kMaxExtent && W <= kMaxExtent;
}

inline long surface_bins(int D, int H, int W) { return (long)(D - 1) * (D - 1) + (long)(H - 1) * (H - 1) + (long)(W - 1) * (W - 1) + 1; }

// classes per chunk: the distance planes of a chunk take about kChunkBytes, whatever C is
inline int chunk_classes(int B, long V) { return (int)std::max<size_t>(1, std::min<size_t>(8, kChunkBytes / (sizeof(int) * (size_t)B * (size_t)V))); }

// the two in-place line passes (along H, then along D) over `planes` volumes of g, every output written
int line_passes(int* g, long planes, int D, int H, int W, hipStream_t st) {
    const long V = (long)D * H * W;
    const int sh = tile_shift(H), sd = tile_shift(D);
    hipLaunchKernelGGL(line_pass_kernel<void>, dim3((W + (1 << sh) - 1) >> sh, D, (unsigned)planes), dim3(256), sizeof(int) * ((size_t)H << sh), st, g, H,
                       (long)W, (long)H * W, W, sh, V, (const void*)nullptr, D, H, 3, 1, 0, 1, 0, (int*)nullptr, 0, (int*)nullptr);
    int rc = pulpo::check_launch("edt line pass H");
    if (rc) return rc;
    hipLaunchKernelGGL(line_pass_kernel<void>, dim3((W + (1 << sd) - 1) >> sd, H, (unsigned)planes), dim3(256), sizeof(int) * ((size_t)D << sd), st, g, D,
                       (long)H * W, (long)W, W, sd, V, (const void*)nullptr, D, H, 3, 1, 0, 1, 0, (int*)nullptr, 0, (int*)nullptr);
    return pulpo::check_launch("edt line pass D");
}

// one direction of one chunk: features = the class surfaces of `feat`, evaluated at the class surfaces of `eval`
template <typename LT>
int surface_direction(const LT* feat, const LT* eval, int* g, int* cnt, int* hist, int* flag, int B, int D, int H, int W, int nd, int CH, int c0, int C,
                      int dir, int bins, hipStream_t st) {
    const long V = (long)D * H * W, planes = (long)B * CH, rows = planes * D * H;
    hipLaunchKernelGGL(row_pass_kernel<LT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const void*)feat, g, rows, D, H, W, nd, CH, c0, C, flag);
    int rc = pulpo::check_launch("surface row pass");
    if (rc) return rc;
    const int sh = tile_shift(H), sd = tile_shift(D);
    hipLaunchKernelGGL(line_pass_kernel<void>, dim3((W + (1 << sh) - 1) >> sh, D, (unsigned)planes), dim3(256), sizeof(int) * ((size_t)H << sh), st, g, H,
                       (long)W, (long)H * W, W, sh, V, (const void*)nullptr, D, H, nd, 1, 0, 1, 0, (int*)nullptr, 0, (int*)nullptr);
    rc = pulpo::check_launch("surface line pass H");
    if (rc) return rc;
    hipLaunchKernelGGL(line_pass_kernel<LT>, dim3((W + (1 << sd) - 1) >> sd, H, (unsigned)planes), dim3(256), sizeof(int) * ((size_t)D << sd), st, g, D,
                       (long)H * W, (long)W, W, sd, V, eval, D, H, nd, CH, c0, C, dir, hist, bins, cnt);
    return pulpo::check_launch("surface line pass D");
}

template <typename LT>
int surface_all(const LT* a, const LT* b, int C, int* g, int* cnt, int* hist, int* flag, int B, int D, int H, int W, int nd, int bins, hipStream_t st) {
    const int CH = chunk_classes(B, (long)D * H * W);
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nc = std::min(CH, C - c0);
        // a short last chunk runs with nc classes per item: the plane index is item * nc + class
        int rc = surface_direction<LT>(b, a, g, cnt, hist, flag, B, D, H, W, nd, nc, c0, C, 0, bins, st);
        if (rc) return rc;
        rc = surface_direction<LT>(a, b, g, cnt, hist, flag, B, D, H, W, nd, nc, c0, C, 1, bins, st);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

PULPO_API int pulpo_edt_sq(const void* mask, int* out, int B, int D, int H, int W, void* stream) {
    PULPO_REQUIRE(mask && out, "edt_sq: null pointer");
    PULPO_REQUIRE(extents_ok(B, D, H, W) && B <= 65535, "edt_sq: extents 1 ... 1024 per axis (depth 1 = 2-D form), B <= 65535");
    PULPO_REQUIRE(((long)B * D * H + 3) / 4 < (1L << 31), "edt_sq: B * D * H beyond the row pass's grid (2^33 rows)");
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * D * H;
    hipLaunchKernelGGL(row_pass_kernel<void>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, mask, out, rows, D, H, W, 3, 1, 0, 1, (int*)nullptr);
    int rc = pulpo::check_launch("edt row pass");
    if (rc) return rc;
    return line_passes(out, B, D, H, W, st);
}

PULPO_API int64_t pulpo_surface_distances_bins(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 ? surface_bins(D, H, W) : 0; }

// layout: [counts (B, C, 2) int32: n_a, n_b][distance planes of one chunk][histograms (B, C, 2, bins), used when the caller passes none: a
// caller that passes its own may hand over a workspace shorter by their 8 B C bins bytes]
PULPO_API size_t pulpo_surface_distances_ws_bytes(int B, int C, int D, int H, int W) {
    if (!extents_ok(B, D, H, W) || C < 1) return 0;
    const size_t V = (size_t)D * H * W;
    return sizeof(int) * (2 * (size_t)B * C + (size_t)B * chunk_classes(B, (long)V) * V + 2 * (size_t)B * C * (size_t)surface_bins(D, H, W));
}

PULPO_API int pulpo_surface_distances(const void* lab_a, const void* lab_b, int ldt, int C, double q, float* out, int* hist, void* ws, int* flag, int B,
                                      int D, int H, int W, int nd, void* stream) {
    PULPO_REQUIRE(lab_a && lab_b && out && ws && flag && (ldt == 0 || ldt == 1) && C >= 1 && C <= (ldt == 0 ? 256 : 65535),
                  "surface_distances: bad arguments (1 <= C, uint8 labels: C <= 256)");
    PULPO_REQUIRE(extents_ok(B, D, H, W) && (nd == 3 || (nd == 2 && D == 1)), "surface_distances: extents 1 ... 1024 per axis; nd = 2 needs depth 1");
    PULPO_REQUIRE(q >= 0.0 && q <= 100.0, "surface_distances: percentile outside [0, 100]");
    const long V = (long)D * H * W, bins = surface_bins(D, H, W);
    const int CH = chunk_classes(B, V);
    PULPO_REQUIRE((long)B * CH <= 65535 && (long)B * C * 2 * bins < (1L << 40) && ((long)B * CH * D * H + 3) / 4 < (1L << 31),
                  "surface_distances: batch too large");
    hipStream_t st = (hipStream_t)stream;
    int* cnt = (int*)ws;
    int* g = cnt + 2 * (size_t)B * C;
    if (hist == nullptr) hist = g + (size_t)B * CH * V;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(int) * 2 * (size_t)B * C, st);
    if (e == hipSuccess) e = hipMemsetAsync(hist, 0, sizeof(int) * 2 * (size_t)B * C * bins, st);
    if (e != hipSuccess) return pulpo::fail((int)e, "surface_distances memset: %s", hipGetErrorString(e));
    int rc = ldt == 0 ? surface_all<uint8_t>((const uint8_t*)lab_a, (const uint8_t*)lab_b, C, g, cnt, hist, flag, B, D, H, W, nd, (int)bins, st)
                      : surface_all<int32_t>((const int32_t*)lab_a, (const int32_t*)lab_b, C, g, cnt, hist, flag, B, D, H, W, nd, (int)bins, st);
    if (rc) return rc;
    hipLaunchKernelGGL(surface_finalize_kernel, dim3(B * C), dim3(256), 0, st, hist, cnt, (int)bins, q, out);
    return pulpo::check_launch("surface_distances finalize");
}
