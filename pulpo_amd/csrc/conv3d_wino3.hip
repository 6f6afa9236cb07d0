// Winograd F(2x2x2, 3x3x3) - minimal filtering in ALL three axes - for the forward / data-gradient convolution: 64 transformed points per
// 2 x 2 x 2 output block instead of the 216 multiply-adds of the direct form (the (y, x) kernel of conv3d_wino2p.hip issues 96): 1.5x fewer
// matrix instructions than that kernel, 3.375x fewer than the direct one, all fp32 (coefficients +-1 and 1/2; measured error against fp64
// 2.8e-7 relative L2 at 32 channels, the (y, x) form 2.1e-7, the direct form 1.2e-7 - same 2e-6 test bound).
//
//   tile 4 x 8 x 8 voxels = 2 x 4 x 4 blocks = ONE 32-row MFMA tile per point; 32 output channels per work item; 8-channel chunks.
//   512 threads = 8 waves, ONE workgroup per CU: wave (py, pzh) owns the eight points (pz in {2 pzh, 2 pzh + 1}, py, px 0..3) - eight
//   32 x 32 accumulator tiles, the register budget of the (y, x) kernel's wave.
//   LDS image of a chunk = the (y, x) kernel's: the halo x-transformed while it is staged (one item per thread: four taps -> four px rows,
//   six raw z planes).  The matrix loop reads four rows per point step - rows ta / tb of planes za / zb - and forms the y AND z
//   combinations in registers (six two-wide fmas); point steps run in pairs whose MFMAs alternate between two accumulator tiles.
//   Staging runs two chunks ahead: the taps a thread requests during chunk c stay in registers for a whole chunk (2000 matrix clocks, more
//   than a trip to HBM) and are transformed into the image of chunk c + 2 at the start of chunk c + 1; two images, one barrier per chunk.
//   Weights global -> registers through a ring of four point rows (a row is re-loaded for the point four steps on as soon as it is used).
//   Epilogue: x inverse transform in registers, the z pair of a wave combined in registers, y (four waves) and the two z halves summed
//   through a 64 KB exchange buffer, one output z parity at a time; stores, bias, BatchNorm partials, the eval-mode store and the fused
//   BatchNorm-backward sums (BNR) as in the (y, x) kernel's fast path.
//
// Whole tiles only (D % 4 == 0, H % 8 == 0, W % 8 == 0), channels-last 16-byte aligned operands, Cin % 8 == 0, Cout % 32 == 0, at least 256 work
// items: every such layer from 16 reduction channels up (pulpo_conv3d_k3_algo = 3; 32 until the end of round 4 - with the leaner tile head and epilogue
// two chunks per tile pay too: 16 -> 96 at 80^3 0.242 -> 0.213 ms).
// What was measured while it was built: an image transformed along x AND z at staging time (two rows per step instead of
// four) multiplies faster (bare loop 0.31 against 0.34 ms at 64 -> 64 / 80^3) but its staging - eight loads, 32 combinations and a second
// item for a quarter of the threads - cost 20 - 24 % against 8 - 10 % here; wave-uniform branches around staging loads cost 15 % (every
// vmcnt behind them becomes a worst-case guess); the plane offset must ride in the VECTOR offset of a buffer load (the bounds check that
// zeroes out-of-volume planes ignores the scalar offset).
#include "conv_shared.h"
#include "conv_epilogue.h"
#include "wino3_pack.h"

namespace {

using namespace pulpo_conv;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int Q_CH = 8, Q_NT = 32;
constexpr int Q_PL = HY * 4;                     // rows of one px slice of a plane: (hy, x-pair)
constexpr int Q_PLROWS = 4 * Q_PL + 2;           // rows per hz plane: the two z blocks of an MFMA row tile lie TWO planes apart = 4 rows mod 16
constexpr int Q_QROWS = 6 * Q_PLROWS;            // rows per channel quad (x 4 dwords = 16 mod 32: the two quads of a ds_write_b128 group use different banks)
constexpr int Q_IMG = 2 * Q_QROWS * 4;           // floats of one image
static_assert((2 * Q_PLROWS) % 16 == 4 && (Q_QROWS * 4) % 32 == 16, "bank layout");
constexpr int Q_NITEM = 6 * HY * 4 * 2;          // staging items of a chunk: (hz, hy, x-pair, channel quad) = 480, one per thread
constexpr int Q_TAB = 3 * 512;                   // per-channel table [3][ncot * 32]: up to 512 output channels
constexpr int Q_R = 8 * 2 * 16 * 64;             // floats of the exchange buffer of one output z parity: [wave][ox][r][lane]
constexpr int Q_RED = 8 * 2 * Q_NT;              // statistics rows of the eight waves
constexpr int Q_PART = 8 * 64 * 8;               // a wave's per-lane statistics before its own (in-order, barrier-free) reduction: [wave][lane][8]
constexpr size_t Q_LDS = (size_t)(2 * Q_IMG + Q_TAB + Q_R + Q_RED + Q_PART) * sizeof(float);
static_assert(Q_LDS <= 160 * 1024, "one workgroup per CU");


// one point row of the packed weights in a lane's registers: four reduction channels of one output channel (32-wide tile), two in the 16-wide form
__device__ __forceinline__ void unpack_w(const float4& w, float (&v)[4]) { v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
__device__ __forceinline__ void unpack_w(const float2& w, float (&v)[4]) { v[0] = w.x; v[1] = w.y; v[2] = 0.f; v[3] = 0.f; }

// SP: the pair of a chunk behind whose first MFMAs a wave transforms and stores its staging item (SP) and requests the next taps (SP + 1)
// N16: the 16-output-channel form (the feedback layers' data gradient, 96 -> 16).  Same tile, chunks, staging, images and barriers; the products
// run on v_mfma_f32_16x16x4_f32 - two per k quad, one per 16-row half of the tile, against a 16-column weight operand - instead of
// 32x32x2 instructions whose upper 16 columns multiply the pack's zero padding: half the matrix clocks.  Lane l = (row i = l % 16, k slot
// kk = l / 16) holds reduction channels 2 kk, 2 kk + 1 of the chunk: it reads EIGHT bytes of row i of each half where the wide form reads
// sixteen of one row (same LDS bytes, the image as store_item writes it), and eight bytes of a weight row.  Accumulators 8 x 2 x 4 registers
// instead of 8 x 16: the room goes to an exchange buffer pass that carries BOTH output z parities at once (16 channels: 2 x 32 KB = the
// buffer), i.e. one barrier pair less per tile, and every thread finishes one voxel pair.
template <bool BNR, int SP, bool N16>
__device__ __forceinline__ void wino3_body(const ConvArgs& a) {
    constexpr int CH = Q_CH, NT = Q_NT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const tab = smem + 2 * Q_IMG;                // [3][ctab]
    float* const R = tab + Q_TAB;                       // exchange buffer
    float* const red = R + Q_R;                         // [8 waves][2][NT]
    float* const part = red + Q_RED;                    // [8 waves][64 lanes][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = N16 ? lane & 15 : lane & 31, kk = N16 ? lane >> 4 : lane >> 5;
    // (N16: wave >> 2 is the copy of the body the wave runs, i.e. SP / 2 - as a constant it takes the issue-priority branches out of the matrix loop:
    //  behind a wave-uniform branch every wait for a load is for ALL loads, the taps just requested included)
    const int py = wave & 3, pzh = N16 ? SP / 2 : wave >> 2;
    const int nchunk = a.Cin / CH;                      // (host: >= 2)
    const int nwork = a.B * a.ntz * a.nty * a.ntx * a.ncot;
    const int nwg = gridDim.x;
    const unsigned ps_bytes = (unsigned)a.in_ps * 4u;
    const unsigned kb_bytes = (unsigned)a.in_kb * 4u;        // bytes between consecutive chunks of a voxel (32: channels-last)

    // ---- the staging item of this thread (the (y, x) kernel's): (hz, hy, x-pair xb, channel quad q) -> the four x-transformed rows px = 0..3
    unsigned roff;                                      // byte offset of tap 0 relative to the tile's halo origin
    int lofs;                                           // float offset of the item's px = 0 row in an image
    {
        const int q = tid & 1, rb = tid >> 1;
        const int xb = rb & 3, hrow = rb >> 2;
        const int hz = hrow / HY, hy = hrow - hz * HY;
        roff = ((unsigned)((hz * a.H + hy) * a.W + 2 * xb) * (unsigned)a.in_ps + 4u * q) * 4u;
        lofs = (q * Q_QROWS + hz * Q_PLROWS + hy * 4 + xb) * 4;
    }
    const bool item = tid < Q_NITEM;
    // combination tables of B^T (rows t_a + s * t_b): point 0: (0, 2, -), 1: (1, 2, +), 2: (2, 1, -), 3: (1, 3, -)
    auto tab_a = [](int p) { return p == 0 ? 0 : p == 2 ? 2 : 1; };
    auto tab_b = [](int p) { return p == 2 ? 1 : p == 3 ? 3 : 2; };
    auto tab_s = [](int p) { return p == 1 ? 1.f : -1.f; };
    // y combination of this wave's point row, z combination of its two point planes pz = 2 pzh + (0, 1): per-wave scalars
    const int ta = tab_a(py), tb = tab_b(py);
    const float sa = tab_s(py);
    // the wave's two z points share THREE planes U, V, W of a z block: pzh = 0: pz 0 = P0 - P2, pz 1 = P1 + P2 (U, V, W = P0, P1, P2);
    // pzh = 1: pz 2 = P2 - P1, pz 3 = P1 - P3 = -(P3 - P1) (U, V, W = P2, P3, P1).  Both waves form  v0 = U - W  and  v1 = V + bw * W  (bw = +1 / -1):
    // the second accumulator of a pzh = 1 wave therefore holds MINUS its point, which the epilogue's z inverse transform takes into account.
    const int zu = (pzh == 0 ? 0 : 2) * Q_PLROWS * 4, zv = (pzh == 0 ? 1 : 3) * Q_PLROWS * 4, zw = (pzh == 0 ? 2 : 1) * Q_PLROWS * 4;
    const float bw = pzh == 0 ? 1.f : -1.f;
    // MFMA row i = block (zb = i >> 4, yb = (i >> 2) & 3, xb = i & 3): halo plane 2 zb + (0..3), halo row 2 yb + (0..3)
    // N16: the tile's 32 rows split into halves by yb / 2, row i of a half = block (zb = i >> 3, yb = 2 half + ((i >> 2) & 1), xb = i & 3): the 16
    // rows of a half then start in 16 different sixteen-byte bank slots (xb + 4 zb + 8 (yb & 1)) and the 32 lanes of a ds_read_b64 group - 16 rows x
    // the two channel pairs of a quad - cover the 64 banks once (halves by zb: rows of yb and yb + 2 share a slot, every read two-way conflicted,
    // measured 0.265 against 0.240 ms for the 32-wide form at 96 -> 16 / 80^3).  Channel quad kk / 2, channel pair kk % 2 of row i; the second half
    // lies A_HALF floats on.
    const int lrow = N16 ? (i >> 3) * 2 * Q_PLROWS + ((i >> 2) & 1) * 8 + (i & 3) : (i >> 4) * 2 * Q_PLROWS + ((i >> 2) & 3) * 8 + (i & 3);
    const int pa_off = N16 ? ((kk >> 1) * Q_QROWS + lrow + ta * 4) * 4 + 2 * (kk & 1) : (kk * Q_QROWS + lrow + ta * 4) * 4;
    const int pb_off = N16 ? ((kk >> 1) * Q_QROWS + lrow + tb * 4) * 4 + 2 * (kk & 1) : (kk * Q_QROWS + lrow + tb * 4) * 4;
    constexpr int A_HALF = 2 * 8 * 4;

    constexpr unsigned OOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, -1, 0x00020000);
    // num_records of the operand's descriptor.  The range check of a raw buffer load is  voffset >= num_records - soffset  (the chunk's offset rides in
    // soffset): the extent must therefore reach the LAST chunk's voxels - in the channel-blocked layout (in_kb = V * 8) that is the whole operand
    const int in_bytes = (int)((((long)a.Cin / CH - 1) * (a.in_kb == CH ? 0 : a.in_kb) + (long)a.D * a.H * a.W * a.in_ps) * 4);
    struct Tile {
        int tile_lin, b, z0, y0, x0, co0;
        unsigned wbase;              // byte offset of (chunk 0, point (2 pzh, py, 0), cout co0) in the packed weights
    };
    auto describe = [&](int work) {
        Tile t;
        const int cot = work % a.ncot;
        int q = work / a.ncot;
        int tx_, ty_, tz_;
        if (a.tile_order == 1) {                        // blocks of 4 x 4 x 4 tiles, as in the (y, x) kernel
            const int nt = a.ntx * a.nty * a.ntz;
            t.b = q / nt;
            q -= t.b * nt;
            const int blk = q >> 6, w = q & 63;
            const int nbx = a.ntx >> 2, nby = a.nty >> 2;
            const int bx = blk % nbx, by = (blk / nbx) % nby, bz = blk / (nbx * nby);
            tx_ = bx * 4 + (w & 3); ty_ = by * 4 + ((w >> 2) & 3); tz_ = bz * 4 + (w >> 4);
        } else {
            tx_ = q % a.ntx; q /= a.ntx;
            ty_ = q % a.nty; q /= a.nty;
            tz_ = q % a.ntz;
            t.b = q / a.ntz;
        }
        t.tile_lin = ((t.b * a.ntz + tz_) * a.nty + ty_) * a.ntx + tx_;
        t.z0 = tz_ * 4; t.y0 = ty_ * TY; t.x0 = tx_ * TX;
        t.co0 = cot * NT;
        t.wbase = (unsigned)(((2 * pzh) * 16 + py * 4) * a.NPad + t.co0) * (CH * 4u);
        return t;
    };
    // byte offsets of this thread's four tap loads of a tile's halo at chunk 0, relative to the batch element; OOB (beyond num_records: the load
    // returns zeros) where the tap lies outside the volume or the item does not exist.  The chunk's channel offset rides in the scalar offset.
    unsigned hoff[4];
    auto halo_offsets = [&](const Tile& t) {
        const unsigned origin = (unsigned)(((t.z0 - 1) * a.H + (t.y0 - 1)) * a.W + (t.x0 - 1)) * ps_bytes;      // modulo 2^32: may be "negative"
        const int rb = tid >> 1;
        const int xb = rb & 3, hrow = rb >> 2;
        const int hz = hrow / HY, hy = hrow - hz * HY;
        const bool rowok = item && (unsigned)(t.z0 - 1 + hz) < (unsigned)a.D && (unsigned)(t.y0 - 1 + hy) < (unsigned)a.H;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
            hoff[tt] = (rowok && (unsigned)(t.x0 - 1 + 2 * xb + tt) < (unsigned)a.W) ? origin + roff + tt * ps_bytes : OOB;
    };
    auto in_rsrc = [&](int b) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + (long)b * a.in_bs), 0, in_bytes, 0x00020000);
    };
    float4 raw[4];                                      // the four x taps of the staging item: loaded one chunk before they are transformed
    auto load_raw = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned c0_bytes, int tt) {
        raw[tt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)hoff[tt], (int)c0_bytes, 0));
    };
    auto store_item = [&](float* img) {
        if (item) {
            float* o = img + lofs;
            const float4 d0 = raw[0], d1 = raw[1], d2 = raw[2], d3 = raw[3];
            *reinterpret_cast<float4*>(o) = make_float4(d0.x - d2.x, d0.y - d2.y, d0.z - d2.z, d0.w - d2.w);
            *reinterpret_cast<float4*>(o + Q_PL * 4) = make_float4(d1.x + d2.x, d1.y + d2.y, d1.z + d2.z, d1.w + d2.w);
            *reinterpret_cast<float4*>(o + 2 * Q_PL * 4) = make_float4(d2.x - d1.x, d2.y - d1.y, d2.z - d1.z, d2.w - d1.w);
            *reinterpret_cast<float4*>(o + 3 * Q_PL * 4) = make_float4(d1.x - d3.x, d1.y - d3.y, d1.z - d3.z, d1.w - d3.w);
        }
    };
    const unsigned w_chunk_stride = 64u * CH * a.NPad * 4u;     // bytes between consecutive chunks
    const unsigned w_pt_stride = (unsigned)CH * a.NPad * 4u;    // bytes between consecutive points (px fastest, then py, then pz)
    const int wl_off = N16 ? (i * CH + 2 * kk) * 4 : (i * CH + 4 * kk) * 4;     // this lane's 16 (N16: 8) bytes inside a point's [32 n][8 k] piece
    using wrow_t = std::conditional_t<N16, float2, float4>;
    auto load_w = [&](unsigned wofs, int s) {                   // point step s = pz_local * 4 + px
        const int so = (int)(wofs + ((s >> 2) * 16 + (s & 3)) * w_pt_stride);
        if constexpr (N16) return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(w_rsrc, wl_off, so, 0));
        else return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, wl_off, so, 0));
    };

    // ---- per-channel constants of the epilogue, once per workgroup
    const int ctab = a.ncot * NT;
    for (int c = tid; c < ctab; c += 512) {
        const bool in = c < a.Cout;
        float t0 = 0.f, t1 = 1.f, t2 = 0.f;
        if (BNR) {
            if (in) { t0 = a.bn_coef[c]; t1 = a.bn_coef[2 * a.Cout + c]; t2 = a.bn_coef[3 * a.Cout + c]; }
        } else {
            if (in && a.bias != nullptr) t0 = a.bias[c];
            if (in && a.coef != nullptr) { t1 = a.coef[2 * a.Cout + c]; t2 = a.coef[3 * a.Cout + c]; }
        }
        tab[c] = t0; tab[ctab + c] = t1; tab[2 * ctab + c] = t2;
    }
    int work = pulpo::xcd_remap(blockIdx.x, nwg);
    Tile cur = describe(work);
    int cb = 0;                                         // image being read
    // ---- prologue: chunk 0 of the first tile staged, chunk 1 requested; the first weight rows
    // N16: a ring of FOUR pairs - a row is re-loaded for the same pair of the NEXT chunk - and the taps are requested in the pair that stores the
    // staging item, not the one after.  Loads return in order: the wait for a weight row requested behind the taps is a wait for the taps.  With
    // 32-clock matrix instructions two pairs are 1000 clocks of the SIMD, less than a trip to HBM under load; a whole chunk is the 2000 clocks the
    // 32-wide form gives them (reasoned from the wait counts in the ISA, not measured on its own: the build it replaced also read through flat
    // loads).  Eight more registers.
    constexpr int WRING = N16 ? 4 : 2;
    wrow_t wr[WRING][2];                                // ring of two pairs of point rows: pair pp uses wr[pp & 1], which then takes pair pp + 2 (N16: see above)
    {
        const __amdgpu_buffer_rsrc_t rs0 = in_rsrc(cur.b);
        halo_offsets(cur);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) load_raw(rs0, 0u, tt);
        store_item(smem);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) load_raw(rs0, kb_bytes, tt);
    }
    // (the weight rows are requested AFTER the taps, as in the loop: the compiler's vmcnt bookkeeping merges this path with the loop's back
    //  edge, and with the taps as the youngest loads here every chunk's transform waited for vmcnt(0) - the weight rows of the pair after next)
    __builtin_amdgcn_sched_barrier(0);                  // (... and the scheduler would hoist them back in front)
#pragma unroll
    for (int pp = 0; pp < WRING; ++pp) { wr[pp][0] = load_w(cur.wbase, pp); wr[pp][1] = load_w(cur.wbase, 4 + pp); }
    __syncthreads();

    float4 ra[3], rb[3];                                // the operand rows of a PAIR of point steps (pz local 0 / 1 at one px): rows ta / tb of planes U, V, W

    // The tile's statistics: the waves' partial sums wait in `red` and are added behind the NEXT barrier every wave passes anyway (the end of the
    // next tile's first chunk, or the one after the loop): the epilogue needs no barrier of its own at its end - the exchange buffer and `red`
    // are not written again before the next tile's epilogue, nchunk barriers away.
    int pend_tile = -1, pend_co0 = 0;
    auto flush_stats = [&]() {
        stats_store<8, NT>(a.stats != nullptr && pend_tile >= 0, red, a.stats, pend_tile, a.Cout, pend_co0, tid);
        pend_tile = -1;
    };
    for (;;) {
        // the next tile is known from the start (its description inside the chunk loop, under `chunk + 2 == nchunk`, was if-converted by the
        // compiler: five integer divisions' worth of scalar instructions and a dozen spilled-register reloads in EVERY chunk)
        const int next_work = work + nwg;
        const bool has_next = next_work < nwork;
        const Tile nxt = has_next ? describe(next_work) : cur;

        constexpr int NH = N16 ? 2 : 1, NR = N16 ? 4 : 16;         // accumulator tiles per point (N16: the two 16-row halves), registers of one
        std::conditional_t<N16, f32x4, f32x16> acc[2][4][NH];   // [pz local][px][half]
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int h = 0; h < NH; ++h)
#pragma unroll
                    for (int r = 0; r < NR; ++r) acc[p][x][h][r] = 0.f;

        unsigned wcur = cur.wbase;                      // weights of the chunk being multiplied
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            // Staging runs TWO chunks ahead of the matrix loop: step 0 transforms the taps requested during the previous chunk into the image
            // of chunk + 1 and steps 1 - 2 request those of chunk + 2 (or of the next tile's chunk 0 / 1), which the registers hold for a whole
            // chunk - 2000 matrix clocks, more than a trip to HBM.
            const bool ahead = chunk + 2 >= nchunk;     // (after the last tile: the tile's own first chunks again, into images nobody reads)
            const unsigned st_c0 = (unsigned)(ahead ? chunk + 2 - nchunk : chunk + 2) * kb_bytes;
            const __amdgpu_buffer_rsrc_t st_rs = in_rsrc(ahead ? nxt.b : cur.b);
            const float* img_r = smem + cb * Q_IMG;
            float* img_w = smem + (cb ^ 1) * Q_IMG;
            const float* pa = img_r + pa_off;
            const float* pb = img_r + pb_off;
            // (N16: the second half's rows through addresses of their own - fused into ds_read2_b64 the pair of reads would run at half the rate, on
            //  32 banks)
            // (the OFFSET is hidden from the compiler, not the pointer: a pointer that has passed through an asm statement is no longer known to point
            //  into the LDS and is read with flat loads, whose waits are for everything)
            int a_half = A_HALF;
            if constexpr (N16) asm volatile("" : "+v"(a_half));
            const float* pa_h = pa + a_half;
            const float* pb_h = pb + a_half;
            auto fetch_a = [&](int px) {
                const int o = px * Q_PL * 4;
                if constexpr (N16) {                    // .xy: channels 2 kk, 2 kk + 1 of row i in half 0, .zw: in half 1
                    auto two = [](const float* p_, const float* h_) {
                        const float2 lo = *reinterpret_cast<const float2*>(p_), hi = *reinterpret_cast<const float2*>(h_);
                        return make_float4(lo.x, lo.y, hi.x, hi.y);
                    };
                    ra[0] = two(pa + zu + o, pa_h + zu + o); rb[0] = two(pb + zu + o, pb_h + zu + o);
                    ra[1] = two(pa + zv + o, pa_h + zv + o); rb[1] = two(pb + zv + o, pb_h + zv + o);
                    ra[2] = two(pa + zw + o, pa_h + zw + o); rb[2] = two(pb + zw + o, pb_h + zw + o);
                    return;
                }
                ra[0] = *reinterpret_cast<const float4*>(pa + zu + o); rb[0] = *reinterpret_cast<const float4*>(pb + zu + o);
                ra[1] = *reinterpret_cast<const float4*>(pa + zv + o); rb[1] = *reinterpret_cast<const float4*>(pb + zv + o);
                ra[2] = *reinterpret_cast<const float4*>(pa + zw + o); rb[2] = *reinterpret_cast<const float4*>(pb + zw + o);
            };
            const bool last_chunk = chunk + 1 == nchunk;
            const unsigned wnext = last_chunk ? (has_next ? nxt.wbase : cur.wbase) : wcur + w_chunk_stride;
            // Point steps run in PAIRS - the wave's two z points at one px: they share the three planes U, V, W (six rows instead of eight), and
            // their MFMAs alternate between two accumulator tiles, so that no matrix instruction waits for the result of the one in front of
            // it.  The rows of the next pair are requested as soon as the combinations have been formed.
            // y combination of each plane (Y = A + sa B), then the two z combinations; two-wide vector arithmetic (v_pk_fma_f32: scalar v_fma_f32
            // measured 3-4 % slower here - the 64-clock fp32 MFMAs leave room)
            auto combine = [&](float (&av0)[4], float (&av1)[4]) {
                const f32x2 sav = {sa, sa}, m1 = {-1.f, -1.f}, bwv = {bw, bw};
                f32x2 ylo[3], yhi[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    ylo[p] = __builtin_elementwise_fma(sav, f32x2{rb[p].x, rb[p].y}, f32x2{ra[p].x, ra[p].y});
                    yhi[p] = __builtin_elementwise_fma(sav, f32x2{rb[p].z, rb[p].w}, f32x2{ra[p].z, ra[p].w});
                }
                const f32x2 lo0 = __builtin_elementwise_fma(m1, ylo[2], ylo[0]), hi0 = __builtin_elementwise_fma(m1, yhi[2], yhi[0]);
                const f32x2 lo1 = __builtin_elementwise_fma(bwv, ylo[2], ylo[1]), hi1 = __builtin_elementwise_fma(bwv, yhi[2], yhi[1]);
                av0[0] = lo0.x; av0[1] = lo0.y; av0[2] = hi0.x; av0[3] = hi0.y;
                av1[0] = lo1.x; av1[1] = lo1.y; av1[2] = hi1.x; av1[3] = hi1.y;
            };
            // Software pipeline over the chunk's four pairs: the operand rows of pair pp + 1 are requested in front of pair pp's MFMAs and
            // COMBINED between them (behind the fourth of the eight), the rows of pair pp + 2 requested right after - a wave never stands in a
            // vector-only phase while it has matrix instructions to issue, except in front of a chunk's first pair.
            float avn0[4], avn1[4];                     // the operands of the pair in flight / of the next pair
            fetch_a(0);
            combine(avn0, avn1);
            // (N16: keeps the px 0 / px 1 requests apart - fused pairwise into ds_read2_b64 they run at half the rate and on 32 banks, two-way conflicted)
            if constexpr (N16) __builtin_amdgcn_sched_barrier(0);
            fetch_a(1);
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                const int s0 = pp, s1 = 4 + pp;         // point steps (pz local 0, px = pp) and (pz local 1, px = pp)
                // The two waves of a SIMD (w and w + 4: pzh 0 / 1) take the higher issue priority in ALTERNATING pairs (+1.5 %; waves 4-7 raised
                // for good gained nothing).  At equal priority the older wave wins every arbitration: it runs its 32 MFMAs of a chunk in 3 350
                // clocks, the younger one gets the leftover slots and finishes alone 1 300 clocks later (in-kernel clock stamps), with the pipe
                // idle in its gaps.
                if (((pp + pzh) & 1) != 0) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
                const float av0[4] = {avn0[0], avn0[1], avn0[2], avn0[3]}, av1[4] = {avn1[0], avn1[1], avn1[2], avn1[3]};
                float wv0[4], wv1[4];
                unpack_w(wr[pp % WRING][0], wv0);
                unpack_w(wr[pp % WRING][1], wv1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
                    if constexpr (N16) {                // step s2 = (k quad ks, half hf): four instructions lie between two on one accumulator
                        const int hf = s2 & 1, ks = s2 >> 1;
                        acc[0][pp][hf] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[2 * hf + ks], wv0[ks], acc[0][pp][hf], 0, 0, 0);
                        acc[1][pp][hf] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[2 * hf + ks], wv1[ks], acc[1][pp][hf], 0, 0, 0);
                    } else {
                        acc[s0 >> 2][s0 & 3][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s2], wv0[s2], acc[s0 >> 2][s0 & 3][0], 0, 0, 0);
                        acc[s1 >> 2][s1 & 3][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s2], wv1[s2], acc[s1 >> 2][s1 & 3][0], 0, 0, 0);
                    }
                    if (s2 == 0) {                      // behind the pair's first MFMAs: the staging work of the pair
                        __builtin_amdgcn_sched_barrier(0);
                        if (pp == SP) {
                            store_item(img_w);
                            if (chunk + 2 == nchunk) halo_offsets(has_next ? nxt : cur);
                        }
                        if (pp == (N16 ? SP : SP + 1)) { load_raw(st_rs, st_c0, 0); load_raw(st_rs, st_c0, 1); load_raw(st_rs, st_c0, 2); load_raw(st_rs, st_c0, 3); }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (s2 == 1 && pp + 1 < 4) {        // behind the fourth MFMA: the next pair's combinations, then the request for the pair after it
                        __builtin_amdgcn_sched_barrier(0);
                        combine(avn0, avn1);
                        __builtin_amdgcn_sched_barrier(0);
                        if (pp + 2 < 4) fetch_a(pp + 2);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // the pair's weights are consumed: a ring of two pairs - the rows take the points of the pair two on (the same chunk's, or the
                // next chunk's first two)
                if constexpr (N16) {
                    wr[pp][0] = load_w(wnext, s0);
                    wr[pp][1] = load_w(wnext, s1);
                } else {
                    wr[pp & 1][0] = pp < 2 ? load_w(wcur, s0 + 2) : load_w(wnext, s0 - 2);
                    wr[pp & 1][1] = pp < 2 ? load_w(wcur, s1 + 2) : load_w(wnext, s1 - 2);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            wcur += w_chunk_stride;
            __syncthreads();                            // image cb ^ 1 complete and visible; every wave has left image cb
            cb ^= 1;
            if (chunk == 0) flush_stats();              // (the previous tile's, see above)
        }

        // ---- epilogue
        float* out_b = a.out + (long)cur.b * a.out_bs;
        const int z0 = cur.z0, y0 = cur.y0, x0 = cur.x0, co0 = cur.co0;
        int elane = lane;
        asm volatile("" : "+v"(elane));
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 s4 = zero4, q4 = zero4;
        const bool fuse = !BNR && a.coef != nullptr;
        if constexpr (N16) {
            // Accumulator register r of half hf in lane l: block (zb = l / 32, yb = 2 hf + (l / 16) % 2, xb = r), output channel l % 16.  The eight
            // waves write their x- and z-inverse-transformed rows of BOTH output z parities into R = [oz][wave][ox][hf * 4 + r][lane] (2 x 32 KB);
            // behind ONE barrier thread (wave = (oz, ox, hf), lane = (xb, zb, yb % 2, channel quad q)) sums the z halves, finishes the y transform
            // and stores its voxel pair (the 16 lanes of a ds_read_b128 group read 64 consecutive floats).
            const int q = elane & 3, vzb = (elane >> 3) & 1, vxb = elane >> 4;
            const int hf_ = wave & 1, ox = (wave >> 1) & 1, oz = wave >> 2;
            const int vyb = 2 * hf_ + ((elane >> 2) & 1);
            const float4 b4 = BNR ? zero4 : *reinterpret_cast<const float4*>(tab + co0 + 4 * q);
            const float4 bm4 = *reinterpret_cast<const float4*>(tab + co0 + 4 * q);
            const float4 sc4 = *reinterpret_cast<const float4*>(tab + ctab + co0 + 4 * q);
            const float4 sh4 = *reinterpret_cast<const float4*>(tab + 2 * ctab + co0 + 4 * q);
            const bool qok = co0 + 4 * q < a.Cout;
            const int gz = z0 + 2 * vzb + oz, gy = y0 + 2 * vyb, gx = x0 + 2 * vxb + ox;
            const long vox = (long)(gz * a.H + gy) * a.W + gx;
            float4 yv0 = zero4, yv1 = zero4;                // BNR: the pre-norm values of the voxel pair, requested in front of the transforms
            if (BNR && qok) {
                const float* bn_b = a.bn_y + (long)cur.b * a.bn_y_bs + co0 + 4 * q;
                yv0 = *reinterpret_cast<const float4*>(bn_b + vox * a.bn_y_ps);
                yv1 = *reinterpret_cast<const float4*>(bn_b + (vox + a.W) * a.bn_y_ps);
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x2 m1 = {-1.f, -1.f};                        // (a - b as fma(m1, b, a): see the 32-wide form below)
            asm volatile("" : "+s"(m1));
            // x inverse transform in place: acc[p][0] <- q0 + q1 + q2, acc[p][1] <- q1 - q2 - q3
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        const f32x2 a0 = {acc[p][0][hf][r], acc[p][0][hf][r + 1]}, a1 = {acc[p][1][hf][r], acc[p][1][hf][r + 1]};
                        const f32x2 a2 = {acc[p][2][hf][r], acc[p][2][hf][r + 1]}, a3 = {acc[p][3][hf][r], acc[p][3][hf][r + 1]};
                        const f32x2 o0 = (a0 + a1) + a2, o1 = __builtin_elementwise_fma(m1, a3, __builtin_elementwise_fma(m1, a2, a1));
                        acc[p][0][hf][r] = o0.x; acc[p][0][hf][r + 1] = o0.y;
                        acc[p][1][hf][r] = o1.x; acc[p][1][hf][r + 1] = o1.y;
                    }
            // z inverse transform, this wave's share (out z0 = q0 + q1 + q2, out z1 = q1 - q2 - q3; pzh = 0 holds (q0, q1), pzh = 1 (q2, -q3))
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float c0 = acc[0][x][hf][r], c1 = acc[1][x][hf][r];
                        float* const w0 = R + (((0 * 8 + wave) * 2 + x) * 8 + hf * 4 + r) * 64 + elane;
                        float* const w1 = R + (((1 * 8 + wave) * 2 + x) * 8 + hf * 4 + r) * 64 + elane;
                        if (pzh == 0) { *w0 = c0 + c1; *w1 = c1; }
                        else { *w0 = c0; *w1 = c1 - c0; }
                    }
            __syncthreads();
            float4 t[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {                   // point row p: the two z halves summed
                const float4 u0 = *reinterpret_cast<const float4*>(R + (((oz * 8 + p) * 2 + ox) * 8 + hf_ * 4 + vxb) * 64 + 4 * (elane & 15));
                const float4 u1 = *reinterpret_cast<const float4*>(R + (((oz * 8 + 4 + p) * 2 + ox) * 8 + hf_ * 4 + vxb) * 64 + 4 * (elane & 15));
                t[p] = make_float4(u0.x + u1.x, u0.y + u1.y, u0.z + u1.z, u0.w + u1.w);
            }
            float4 v0, v1;
            inverse_last(t[0], t[1], t[2], t[3], b4, v0, v1);
            if (BNR) bn_bwd_reduce_pair(v0, v1, yv0, yv1, sc4, sh4, bm4, a.slope, s4, q4);
            else stats_add_pair(v0, v1, s4, q4);
            if (fuse) {
                v0 = bn_lrelu4(v0, sc4, sh4, a.slope);
                v1 = bn_lrelu4(v1, sc4, sh4, a.slope);
            }
            float* obase = out_b + (long)((co0 + 4 * q) >> 3) * a.out_kb + ((4 * q) & 7);
            if (qok) {
                *reinterpret_cast<float4*>(obase + vox * a.out_ps) = v0;
                *reinterpret_cast<float4*>(obase + (vox + a.W) * a.out_ps) = v1;
            }
            // per-tile partial sums: lane l owns ONE of the wave's sums (which = l / 32, channel l % 32 < 16) and adds the sixteen lanes q + 4 j
            // that hold its channel quad, through the wave's own LDS rows (in order, no barrier)
            if (a.stats != nullptr) {
                float* pw_ = part + (wave * 64 + elane) * 8;
                *reinterpret_cast<float4*>(pw_) = s4;
                *reinterpret_cast<float4*>(pw_ + 4) = q4;
                const int c_ = elane & 31, wh_ = elane >> 5;
                const float* pr_ = part + (wave * 64 + ((c_ >> 2) & 3)) * 8 + wh_ * 4 + (c_ & 3);
                float t_ = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) t_ += pr_[j * 32];         // lanes q + 4 j
                red[(wave * 2 + wh_) * NT + c_] = c_ < 16 ? t_ : 0.f;
            }
        } else {
            const int q = elane & 7, kh = (elane >> 3) & 1, g = elane >> 4;
            const float4 b4 = BNR ? zero4 : *reinterpret_cast<const float4*>(tab + co0 + 4 * q);
            const float4 bm4 = *reinterpret_cast<const float4*>(tab + co0 + 4 * q);
            const float4 sc4 = *reinterpret_cast<const float4*>(tab + ctab + co0 + 4 * q);
            const float4 sh4 = *reinterpret_cast<const float4*>(tab + 2 * ctab + co0 + 4 * q);
            const float* bn_b = BNR ? a.bn_y + (long)cur.b * a.bn_y_bs + co0 + 4 * q : nullptr;
            // this lane finishes (ox, r) = combo of the exchange buffer, rows of half kh, channels 4 q .. 4 q + 3
            const int combo = wave * 4 + g;
            const int ox = combo >> 4, rr = combo & 15;
            const int row = (rr & 3) + 8 * (rr >> 2) + 4 * kh;          // = MFMA row = block (zb, yb, xb)
            const int vzb = row >> 4, vyb = (row >> 2) & 3, vxb = row & 3;
            // x inverse transform (4 px -> 2 ox), once and in place: acc[p][0] <- out x0 = q0 + q1 + q2, acc[p][1] <- out x1 = q1 - q2 - q3
            // BNR: the pre-norm values of this lane's two output voxels of a parity are requested EARLY - parity 0 in front of the x inverse transform,
            // parity 1 as soon as parity 0's have been used - so that a miss (y is read once per step: HBM) lands under the transform and the exchange
            // instead of in front of the sums that need it
            float4 yv0 = zero4, yv1 = zero4;
            const bool qok = co0 + 4 * q < a.Cout;         // (a partly empty cout tile: channel quads beyond the tensor are neither read nor stored)
            auto load_y = [&](int oz_) {
                if (BNR && qok) {
                    const long vox_ = (long)((z0 + 2 * vzb + oz_) * a.H + y0 + 2 * vyb) * a.W + x0 + 2 * vxb + ox;
                    yv0 = *reinterpret_cast<const float4*>(bn_b + vox_ * a.bn_y_ps);
                    yv1 = *reinterpret_cast<const float4*>(bn_b + (vox_ + a.W) * a.bn_y_ps);
                }
            };
            load_y(0);
            __builtin_amdgcn_sched_barrier(0);
            // a - b below is fma(m1, b, a) with m1 = -1 the compiler cannot see through: exact (the product is), and it stays ONE two-wide instruction
            // (v_pk_fma_f32) - a two-wide subtraction is expanded into two scalar ones by the backend
            f32x2 m1 = {-1.f, -1.f};
            asm volatile("" : "+s"(m1));
            // (two-wide: the accumulator registers of rows r, r + 1 are an aligned pair - v_pk_add_f32 with the association of the scalar form,
            //  (a0 + a1) + a2 and (a1 - a2) - a3: 64 instead of 128 vector instructions per wave, which the SIMD's two waves issue at the same time)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2 a0 = {acc[p][0][0][r], acc[p][0][0][r + 1]}, a1 = {acc[p][1][0][r], acc[p][1][0][r + 1]};
                    const f32x2 a2 = {acc[p][2][0][r], acc[p][2][0][r + 1]}, a3 = {acc[p][3][0][r], acc[p][3][0][r + 1]};
                    const f32x2 o0 = (a0 + a1) + a2, o1 = __builtin_elementwise_fma(m1, a3, __builtin_elementwise_fma(m1, a2, a1));
                    acc[p][0][0][r] = o0.x; acc[p][0][0][r + 1] = o0.y;
                    acc[p][1][0][r] = o1.x; acc[p][1][0][r + 1] = o1.y;
                }
#pragma unroll
            for (int oz = 0; oz < 2; ++oz) {
                if (oz > 0) __syncthreads();                // every wave has left the exchange buffer (previous parity)
                // this wave's share of the z inverse transform: out z0 = q0 + q1 + q2, out z1 = q1 - q2 - q3; wave pzh = 0 holds (q0, q1), pzh = 1
                // holds (q2, -q3) (the second accumulator of those waves holds MINUS its point, see the matrix loop).  A branch per wave (pzh is
                // wave-uniform) instead of two selects per value.
                float* const r0 = R + ((wave * 2 + 0) * 16) * 64 + elane;
                float* const r1 = R + ((wave * 2 + 1) * 16) * 64 + elane;
                if (pzh == 0) {
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2 u0 = f32x2{acc[0][0][0][r], acc[0][0][0][r + 1]} + f32x2{acc[1][0][0][r], acc[1][0][0][r + 1]};
                        const f32x2 u1 = f32x2{acc[0][1][0][r], acc[0][1][0][r + 1]} + f32x2{acc[1][1][0][r], acc[1][1][0][r + 1]};
                        r0[r * 64] = oz == 0 ? u0.x : acc[1][0][0][r]; r0[(r + 1) * 64] = oz == 0 ? u0.y : acc[1][0][0][r + 1];
                        r1[r * 64] = oz == 0 ? u1.x : acc[1][1][0][r]; r1[(r + 1) * 64] = oz == 0 ? u1.y : acc[1][1][0][r + 1];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2 u0 = __builtin_elementwise_fma(m1, f32x2{acc[0][0][0][r], acc[0][0][0][r + 1]}, f32x2{acc[1][0][0][r], acc[1][0][0][r + 1]});
                        const f32x2 u1 = __builtin_elementwise_fma(m1, f32x2{acc[0][1][0][r], acc[0][1][0][r + 1]}, f32x2{acc[1][1][0][r], acc[1][1][0][r + 1]});
                        r0[r * 64] = oz == 0 ? acc[0][0][0][r] : u0.x; r0[(r + 1) * 64] = oz == 0 ? acc[0][0][0][r + 1] : u0.y;
                        r1[r * 64] = oz == 0 ? acc[0][1][0][r] : u1.x; r1[(r + 1) * 64] = oz == 0 ? acc[0][1][0][r + 1] : u1.y;
                    }
                }
                const int gz = z0 + 2 * vzb + oz, gy = y0 + 2 * vyb, gx = x0 + 2 * vxb + ox;
                const long vox = (long)(gz * a.H + gy) * a.W + gx;
                __syncthreads();
                float4 t[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {               // point row p: the two z halves summed
                    const float4 u0 = *reinterpret_cast<const float4*>(R + (((0 * 4 + p) * 2 + ox) * 16 + rr) * 64 + kh * 32 + 4 * q);
                    const float4 u1 = *reinterpret_cast<const float4*>(R + (((1 * 4 + p) * 2 + ox) * 16 + rr) * 64 + kh * 32 + 4 * q);
                    t[p] = make_float4(u0.x + u1.x, u0.y + u1.y, u0.z + u1.z, u0.w + u1.w);
                }
                float4 v0, v1;
                inverse_last(t[0], t[1], t[2], t[3], b4, v0, v1);
                if (BNR) {
                    bn_bwd_reduce_pair(v0, v1, yv0, yv1, sc4, sh4, bm4, a.slope, s4, q4);     // (pulpo::bn_bwd_reduce_step, head_bn.h)
                    if (oz == 0) { __builtin_amdgcn_sched_barrier(0); load_y(1); __builtin_amdgcn_sched_barrier(0); }
                } else {
                    stats_add_pair(v0, v1, s4, q4);
                }
                if (fuse) {
                    v0 = bn_lrelu4(v0, sc4, sh4, a.slope);
                    v1 = bn_lrelu4(v1, sc4, sh4, a.slope);
                }
                float* obase = out_b + (long)((co0 + 4 * q) >> 3) * a.out_kb + ((4 * q) & 7);      // (out_kb = 8: channels-last, co0 + 4 q)
                if (qok) {
                    *reinterpret_cast<float4*>(obase + vox * a.out_ps) = v0;
                    *reinterpret_cast<float4*>(obase + (vox + a.W) * a.out_ps) = v1;
                }
            }
            // per-tile BatchNorm partial sums: over the lanes that hold the same channels, then over the eight waves
            // (through the wave's own LDS rows - DS operations of one wave execute in order, no barrier - instead of three rounds of cross-lane
            //  shuffles: lane l then owns ONE of the wave's 64 sums (which = l / 32, channel l % 32) and adds the eight lanes that hold its channel quad)
            if (a.stats != nullptr) {
                float* pw_ = part + (wave * 64 + elane) * 8;
                *reinterpret_cast<float4*>(pw_) = s4;
                *reinterpret_cast<float4*>(pw_ + 4) = q4;
                const int c_ = elane & 31, wh_ = elane >> 5;
                const float* pr_ = part + (wave * 64 + (c_ >> 2)) * 8 + wh_ * 4 + (c_ & 3);
                float t_ = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) t_ += pr_[j * 64];          // lanes q + 8 j
                red[(wave * 2 + wh_) * NT + c_] = t_;
            }
        }
        pend_tile = cur.tile_lin; pend_co0 = co0;
        if (!has_next) break;
        cur = nxt;
        work = next_work;
    }
    __syncthreads();
    flush_stats();
}

// The kernel body exists in two copies that differ in ONE constant, SP.  Waves 0-3 stage behind pairs 0 / 1 of a chunk, their SIMD partners 4-7
// behind pairs 2 / 3: the kernel's phases ADD UP (ablations, DESIGN 3d: two waves per SIMD in lock step hide nothing of each other) - staggered,
// one wave's vector and LDS-write work falls into the other's matrix phase.  Two whole copies behind ONE wave-uniform branch at the top (no state
// joins behind it: the copies share only the kernel arguments and the LDS), and a compile-time constant per copy, because a wave-uniform RUNTIME
// branch around the tap loads makes every vmcnt behind it a worst-case guess (measured in round 4: -15 %).  Both copies pass the same barriers.
template <bool BNR, bool N16>
__global__ __launch_bounds__(512, 1) void conv3d_k3_wino3_mfma(ConvArgs a) {
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 8) != 0) wino3_body<BNR, 2, N16>(a);
    else wino3_body<BNR, 0, N16>(a);
}

__global__ void pack_weight_wino3_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int NPad, int dgrad, long total) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
        pulpo_conv::pack_wino3_one(w, wp, Cin, Cout, NPad, dgrad, e);
}

// smallest reduction-channel count that takes this kernel (at least two chunks per tile: the statistics' deferred flush counts on a second
// chunk barrier)
constexpr int WINO3_MIN_K = 16;

}  // namespace

namespace pulpo_conv {

// shapes the F(2x2x2,3x3x3) kernel takes: whole 4 x 8 x 8 tiles, K % 8 == 0, N % 32 == 0, at least 256 work items (one per CU)
int wino3_shape_ok(int B, int D, int H, int W, int K, int N) {
    // (output channels: a multiple of 4; a cout tile of 32 may be partly empty.  The 16-channel data gradient of the feedback layer is admitted
    //  as before and runs the kernel's 16-column form: pulpo_conv3d_k3_narrow16)
    const int ncot = (N + Q_NT - 1) / Q_NT;
    if (K < WINO3_MIN_K || K % Q_CH != 0 || N % 4 != 0 || (N % Q_NT != 0 && N < 16) || 3 * ncot * Q_NT > Q_TAB) return 0;
    if (D % 4 != 0 || H % TY != 0 || W % TX != 0) return 0;
    // the BatchNorm statistics rows are counted by pulpo_conv3d_k3_stat_tiles(), i.e. with conv_tz(): this kernel writes one row per 4-deep tile
    if (conv_tz(D, H, W) != 4) return 0;
    const long items = (long)B * (D / 4) * (H / TY) * (W / TX) * ncot;
    return items >= 256;
}

}  // namespace pulpo_conv

// which form of a kernel a channel pair runs (read-only; the launchers decide through it).  kind 0: the forward / data-gradient F(2x2x2,3x3x3)
// kernel with K reduction and N output channels - 1: the 16-column form on v_mfma_f32_16x16x4_f32 (N == 16), 0: the 32-wide cout tiles.
// kind 1: the F(2x2x2,3x3x3) weight-gradient kernel (conv3d_wgrad_w2.hip) with K = Cin, N = Cout - 1: the last ci tile holds 16 channels
// (Cin % 32 == 16) and its workgroups run the 16-row form, 0: 32-row tiles only.  Any other kind: 0.
PULPO_API int pulpo_conv3d_k3_narrow16(int kind, int K, int N) {
    if (kind == 0) return K >= WINO3_MIN_K && K % Q_CH == 0 && N == 16;
    if (kind == 1) return K > 0 && N > 0 && K % 32 == 16;
    return 0;
}

PULPO_API size_t pulpo_conv3d_k3_packed_wino3_floats(int K, int N) { return (size_t)((K + Q_CH - 1) / Q_CH) * 64 * Q_CH * npad(N); }

PULPO_API int pulpo_conv3d_k3_pack_weight_wino3(const float* w, float* wp, int Cin, int Cout, int dgrad, void* stream) {
    PULPO_REQUIRE(w && wp && Cin > 0 && Cout > 0, "conv3d_k3_pack_weight_wino3: bad arguments");
    const int K = dgrad ? Cout : Cin, N = dgrad ? Cin : Cout;
    const long total = (long)((K + Q_CH - 1) / Q_CH) * Q_CH * npad(N);          // threads: one per (chunk, k, n)
    const int nb = (int)std::min<long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(pack_weight_wino3_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, w, wp, Cin, Cout, npad(N), dgrad, total);
    return pulpo::check_launch("pack_weight_wino3");
}

static int fwd_wino3_impl(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias, const float* coef, float slope,
                          float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps,
                          const float* bn_coef, int B, int D, int H, int W, int K, int N, void* stream, int64_t in_kb = Q_CH, int64_t out_kb = Q_CH) {
    PULPO_REQUIRE(in && wp && out, "conv3d_k3_fwd_wino3: null pointer");
    PULPO_REQUIRE(B > 0 && K > 0 && N > 0 && D > 0 && D % 4 == 0 && H > 0 && H % TY == 0 && W > 0 && W % TX == 0 && K % Q_CH == 0 && N % 4 == 0 && 3 * ((N + Q_NT - 1) / Q_NT) * Q_NT <= Q_TAB,
                  "conv3d_k3_fwd_wino3: shape %dx%dx%d, %d -> %d channels is not whole 4x8x8 tiles of 8 / 32 channels (see pulpo_conv3d_k3_algo)", D, H, W, K, N);
    PULPO_REQUIRE(K >= 2 * Q_CH, "conv3d_k3_fwd_wino3: at least two 8-channel chunks per tile (%d reduction channels given): the staging runs two chunks ahead", K);
    PULPO_REQUIRE(!stats || conv_tz(D, H, W) == 4, "conv3d_k3_fwd_wino3: %dx%dx%d is tiled 2-deep by pulpo_conv3d_k3_stat_tiles(); this kernel writes 4-deep statistics rows", D, H, W);
    PULPO_REQUIRE(!(coef && stats), "conv3d_k3_fwd_wino3: batch statistics are not available from the fused eval-mode epilogue");
    PULPO_REQUIRE(in_cs == 1 && in_ps % 4 == 0 && in_bs % 4 == 0 && (((uintptr_t)in) & 15) == 0 && (long)D * H * W * in_ps * 4 < (1L << 31) &&
                      in_kb >= Q_CH && in_kb % 4 == 0 && ((long)(K / Q_CH - 1) * in_kb + (long)D * H * W * in_ps) * 4 < (1L << 31),
                  "conv3d_k3_fwd_wino3: the operand must be channels-last (or channel-blocked), 16-byte aligned and smaller than 2 GiB per batch element");
    PULPO_REQUIRE(out_cs == 1 && out_ps % 4 == 0 && out_bs % 4 == 0 && (((uintptr_t)out) & 15) == 0, "conv3d_k3_fwd_wino3: the result must be channels-last, 16-byte aligned");
    PULPO_REQUIRE((((uintptr_t)wp) & 15) == 0, "conv3d_k3_fwd_wino3: packed weights must be 16-byte aligned");
    PULPO_REQUIRE(out_kb >= Q_CH && out_kb % 4 == 0 && (out_kb == Q_CH || N % Q_CH == 0), "conv3d_k3_fwd_wino3: a channel-blocked result needs whole 8-channel blocks");
    ConvArgs a{};
    a.in = in; a.in_bs = in_bs; a.in_ps = in_ps; a.in_cs = in_cs; a.in_kb = in_kb; a.out_kb = out_kb;
    a.wp = wp; a.bias = bias;
    a.out = out; a.out_bs = out_bs; a.out_ps = out_ps; a.out_cs = out_cs;
    a.stats = stats;
    a.coef = coef; a.slope = slope;
    a.bn_y = bn_y; a.bn_y_bs = bn_y_bs; a.bn_y_ps = bn_y_ps; a.bn_coef = bn_coef;
    a.B = B; a.D = D; a.H = H; a.W = W; a.Cin = K; a.Cout = N; a.NPad = npad(N);
    a.ntz = D / 4; a.nty = H / TY; a.ntx = W / TX;
    a.ncot = (N + Q_NT - 1) / Q_NT;
    a.ksplit = 1; a.part = nullptr;
    a.tile_order = (a.ntx % 4 == 0 && a.nty % 4 == 0 && a.ntz % 4 == 0) ? 1 : 0;
    const long nwork = (long)B * a.ntz * a.nty * a.ntx * a.ncot;
    PULPO_REQUIRE(nwork < (1L << 31), "conv3d_k3_fwd_wino3: grid too large");
    hipStream_t st = (hipStream_t)stream;
    const bool bnr = bn_y != nullptr;
    const bool n16 = pulpo_conv3d_k3_narrow16(0, K, N) != 0;     // 16 output channels: the 16x16x4 form of the kernel
    using kernel_t = void (*)(ConvArgs);
    static const kernel_t kernels[2][2] = {{conv3d_k3_wino3_mfma<false, false>, conv3d_k3_wino3_mfma<false, true>},
                                           {conv3d_k3_wino3_mfma<true, false>, conv3d_k3_wino3_mfma<true, true>}};
    static bool attr_set[2][2] = {{false, false}, {false, false}};
    const kernel_t fn = kernels[bnr][n16];
    if (!attr_set[bnr][n16]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Q_LDS);
        if (e != hipSuccess) return pulpo::fail((int)e, "hipFuncSetAttribute(conv3d wino3): %s", hipGetErrorString(e));
        attr_set[bnr][n16] = true;
    }
    const int nwg = (int)std::min<long>(nwork, 256);    // persistent workgroups: one per CU
    hipLaunchKernelGGL(fn, dim3(nwg), dim3(512), Q_LDS, st, a);
    return pulpo::check_launch("conv3d_k3_wino3_mfma");
}

PULPO_API int pulpo_conv3d_k3_fwd_wino3(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias,
                                        const float* coef, float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, int B,
                                        int D, int H, int W, int K, int N, void* stream) {
    return fwd_wino3_impl(in, in_bs, in_ps, in_cs, wp, bias, coef, slope, out, out_bs, out_ps, out_cs, stats, nullptr, 0, 0, nullptr, B, D, H, W, K, N, stream);
}

PULPO_API int pulpo_conv3d_k3_dgrad_wino3_bnred(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, float* out, int64_t out_bs,
                                                int64_t out_ps, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps, const float* bn_coef, float slope,
                                                float* part, int B, int D, int H, int W, int K, int N, void* stream) {
    PULPO_REQUIRE(bn_y && bn_coef && part, "conv3d_k3_dgrad_wino3_bnred: null pointer");
    PULPO_REQUIRE(bn_y_ps % 4 == 0 && bn_y_bs % 4 == 0 && (((uintptr_t)bn_y) & 15) == 0 && (((uintptr_t)bn_coef) & 15) == 0,
                  "conv3d_k3_dgrad_wino3_bnred: pre-norm tensor and coefficients must be channels-last and 16-byte aligned");
    return fwd_wino3_impl(in, in_bs, in_ps, in_cs, wp, nullptr, nullptr, slope, out, out_bs, out_ps, 1, part, bn_y, bn_y_bs, bn_y_ps, bn_coef, B, D, H, W, K, N,
                          stream);
}

// The same two kernels on a channel-BLOCKED operand: element (voxel v, channel c) at  in + b * in_bs + (c / 8) * in_kb + v * in_ps + c % 8  (floats).
// in_kb = 8, in_ps = row pitch is the channels-last tensor of the entries above; in_kb = D * H * W * 8, in_ps = 8 is the layout [K / 8][D][H][W][8], in
// which the four taps of a staging item are 128 consecutive bytes and a wave's tap load touches a fifth of the cache lines.
PULPO_API int pulpo_conv3d_k3_fwd_wino3_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* wp, const float* bias,
                                           const float* coef, float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_kb, float* stats, int B,
                                           int D, int H, int W, int K, int N, void* stream) {
    return fwd_wino3_impl(in, in_bs, in_ps, 1, wp, bias, coef, slope, out, out_bs, out_ps, 1, stats, nullptr, 0, 0, nullptr, B, D, H, W, K, N, stream, in_kb,
                          out_kb);
}

PULPO_API int pulpo_conv3d_k3_dgrad_wino3_bnred_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* wp, float* out, int64_t out_bs,
                                                   int64_t out_ps, int64_t out_kb, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps, const float* bn_coef, float slope,
                                                   float* part, int B, int D, int H, int W, int K, int N, void* stream) {
    PULPO_REQUIRE(bn_y && bn_coef && part, "conv3d_k3_dgrad_wino3_bnred_kb: null pointer");
    PULPO_REQUIRE(bn_y_ps % 4 == 0 && bn_y_bs % 4 == 0 && (((uintptr_t)bn_y) & 15) == 0 && (((uintptr_t)bn_coef) & 15) == 0,
                  "conv3d_k3_dgrad_wino3_bnred_kb: pre-norm tensor and coefficients must be channels-last and 16-byte aligned");
    return fwd_wino3_impl(in, in_bs, in_ps, 1, wp, nullptr, nullptr, slope, out, out_bs, out_ps, 1, part, bn_y, bn_y_bs, bn_y_ps, bn_coef, B, D, H, W, K, N,
                          stream, in_kb, out_kb);
}
