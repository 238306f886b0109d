// The ResNet stem and its max-pool in one launch (bf16, 64 output channels):
//   Conv2d(3, 64, 7, stride 2, padding 3) + folded BN shift + ReLU   model/resnet.py:111-113  (pixel-paired form, conv_igemm.hip cs_stem_*)
//   MaxPool2d(3, 2, 1)                                               model/resnet.py:114      (pool.hip maxpool_fwd_kernel)
// cs_stem_fwd_packed writes the [N][P][Q][64] stem map and cs_maxpool3x3s2_fwd reads it back; nothing else ever looks at that map
// (184 MB each way on the ResNet-50 tile step).  Here a workgroup takes TP x TQ tiles of POOLED outputs, one after the other, with
// the paired weights [64][7][4][8] in registers throughout (14 fragments per wave); per tile:
//   1. the input window of the tile -- (4 TP + 7) rows of (2 TQ + 4) 16-byte pixel pairs, zeros outside the image -- goes to LDS
//      (fetched into registers while the previous tile was being computed);
//   2. the (2 TP + 1) x (2 TQ + 1) stem outputs under the tile's pool windows are computed with v_mfma_f32_32x32x16_bf16: one extra
//      row and column per tile are recomputed so that no window crosses a tile.  The pixel fragment of slot (kh, pw) is ONE
//      ds_read_b128 straight from the window (row 2 ly + kh, pair lx + pw of local stem pixel (ly, lx)): no im2col copy;
//   3. shift, one rounding to bf16, ReLU -> an LDS tile of stem values;
//   4. the tile is pooled and y_pool (8 bytes) / the tap bytes (4 bytes) of 4 channels are stored per thread.
// The values are those of the two launches it replaces, bit for bit:
//   * contraction: slots 0..27 in order, two per 16-deep MFMA (lanes 0-31 the even slot, 32-63 the odd one), weights as source A and
//     pixels as source B, from a zero accumulator -- the ring kernel's walk over its gathered rows (conv_v2.hip conv2_ring_kernel GA;
//     its slots 28..31 are zero on both sides and add nothing);
//   * epilogue: accumulator + shift in fp32, v_cvt_pk_bf16_f32, ReLU on the packed pair (conv_v2.hip pack_tile);
//   * pool: the ROUNDED values, taps scanned kh-major, a tap taken if strictly greater or NaN, the first valid tap seeds the maximum,
//     taps outside the stem map skipped (pool.hip maxpool_fwd_kernel).
#include <algorithm>
#include "cs_common.h"

namespace {

#ifndef CS_STEM_POOL_TP
#define CS_STEM_POOL_TP 5          // 75 = 15 x 5 and 75 = 5 x 15: no ragged tile on the 299 x 299 tiles of the classifier
#define CS_STEM_POOL_TQ 15
#endif

struct SpParams {
    const uint4* x;                // [N][H][Wh] pixel pairs
    const uint4* w;                // [64][28] slots of 8 bf16
    const float* shift;            // [64] or NULL
    bf16_t* y;                     // [N][PP][PQ][64]
    uint8_t* amax;                 // [N][PP][PQ][64] or NULL
    int H, Wh, P, Q, PP, PQ;
    unsigned N, tiles_x, tiles_y;
};

template <int TP, int TQ> struct SpTile {
    static constexpr int SH = 2 * TP + 1, SW = 2 * TQ + 1;       // stem outputs of the tile
    static constexpr int NPIX = SH * SW, NT = (NPIX + 31) / 32;  // ... as 32-pixel MFMA tiles
    static constexpr int NTW = (NT + 1) / 2;                     // per wave: waves 0/1 take the even pixel tiles, 2/3 the odd ones
    static constexpr int WR = 4 * TP + 7, WP = 2 * TQ + 4;       // input window: rows, pairs
    static constexpr int NW = (WR * WP + 255) / 256;             // 16-byte window loads per thread; the LDS window is padded to whole rounds
    static constexpr unsigned WIN_BYTES = (unsigned)NW * 4096u;
    static constexpr unsigned ROW = 144u;                        // bytes per stem pixel in LDS: 128 + 16, so that 8 consecutive pixel lanes' 16-byte writes fall into distinct banks
    static constexpr unsigned TILE_BYTES = (unsigned)NPIX * ROW;
    static constexpr unsigned LDS = WIN_BYTES + TILE_BYTES;
    static_assert(LDS <= 81920u, "two workgroups per compute unit");
    static_assert(6 * WP * 16 + 32 < 65536, "ds_read immediate offset");
};

__device__ __forceinline__ void swap_halves(unsigned& a, unsigned& b) {
    // lanes 32-63 of a <-> lanes 0-31 of b
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

template <int TP, int TQ>
__global__ __launch_bounds__(256, 2) void stem_pool_fwd_kernel(SpParams p) {
    using T = SpTile<TP, TQ>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const win = smem;
    unsigned char* const til = smem + T::WIN_BYTES;          // the tile of stem values

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    // this wave: channels [32 ct, 32 ct + 32) of pixel tiles tw, tw + 2, ...
    const int ct = wave & 1, tw = wave >> 1;

    // The workgroup is persistent: it walks every gridDim.x-th tile and keeps in registers what does not change from tile to tile --
    // the weight fragment of each 16-deep step j (filter row 32 ct + l31, slot 2 j + hh) and the shift of accumulator register r
    // (channel 32 ct + 8 (r >> 2) + 4 hh + (r & 3)).  (A first version ran one tile per workgroup and staged the weights through LDS:
    // the two workgroups of a compute unit marched in step -- both loading, both multiplying, both pooling -- and the launch took the
    // SUM of its phases, 118 us.)
    bf16x8 bw[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) bw[j] = __builtin_bit_cast(bf16x8, p.w[(ct * 32 + l31) * 28 + 2 * j + hh]);
    float sh[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.shift) s4 = *reinterpret_cast<const float4*>(p.shift + ct * 32 + 8 * g + 4 * hh);
        sh[4 * g] = s4.x; sh[4 * g + 1] = s4.y; sh[4 * g + 2] = s4.z; sh[4 * g + 3] = s4.w;
    }
    // pixel l31 of pixel tile t is local stem pixel t * 32 + l31 in row-major order; past the tile: pixel 0, computed and dropped.
    // (An odd tile count: waves 2/3 have one tile less than waves 0/1 and compute pixel 0 in its place -- they sit on SIMDs of their
    // own and would wait for waves 0/1 anyway; a branch would cut the main loop into 14 scheduling regions.)
    unsigned abase[T::NTW];
#pragma unroll
    for (int ti = 0; ti < T::NTW; ++ti) {
        const int pi = (tw + 2 * ti) * 32 + l31;
        const int pc = pi < T::NPIX ? pi : 0;
        const int ly = pc / T::SW, lx = pc - ly * T::SW;
        abase[ti] = (unsigned)((2 * ly * T::WP + lx + hh) * 16);
    }

    // ---- 1. the window of a tile, global -> registers.  Local stem pixel (0, 0) is stem pixel (2 p0 - 1, 2 q0 - 1): tap (0, 0) of
    // pooled (p0, q0); its slot (0, 0) is input row 2 (2 p0 - 1) - 3, pair (2 q0 - 1) - 2.  No load sits under a branch (the compiler
    // waits for such loads one by one): a pair outside the image reads pair 0 of the image and is zeroed when it is written to LDS.
    // The loads of tile t + 1 are issued in front of the main loop of tile t and land behind its MFMAs, its epilogue and its pool.
    const unsigned n_tiles = p.tiles_x * p.tiles_y * p.N;
    uint4 wv[T::NW];
    unsigned wok = 0u;
    auto fetch = [&](unsigned tile) {
        const unsigned tx = tile % p.tiles_x, r1 = tile / p.tiles_x;
        const unsigned ty = r1 % p.tiles_y;
        const size_t n = r1 / p.tiles_y;
        const int iy0 = 4 * (int)ty * TP - 5, px0 = 2 * (int)tx * TQ - 3;
        const uint4* xi = p.x + n * (size_t)p.H * (size_t)p.Wh;
        wok = 0u;
#pragma unroll
        for (int k = 0; k < T::NW; ++k) {
            const int i = tid + 256 * k;
            const int r = i / T::WP, c = i - r * T::WP;
            const int iy = iy0 + r, px = px0 + c;
            const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)px < (unsigned)p.Wh;       // (rows past the window: never read)
            wv[k] = xi[ok ? (size_t)iy * (size_t)p.Wh + (size_t)px : (size_t)0];
            wok |= ok ? 1u << k : 0u;
        }
    };
    unsigned tile = blockIdx.x;
    if (tile < n_tiles) fetch(tile);
    for (; tile < n_tiles; tile += gridDim.x) {
        const unsigned tx = tile % p.tiles_x, r1 = tile / p.tiles_x;
        const unsigned ty = r1 % p.tiles_y;
        const size_t n = r1 / p.tiles_y;
        const int p0 = (int)ty * TP, q0 = (int)tx * TQ;      // first pooled output of the tile
#pragma unroll
        for (int k = 0; k < T::NW; ++k)
            reinterpret_cast<uint4*>(win)[tid + 256 * k] = (wok >> k) & 1u ? wv[k] : make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();             // the window is there; the pool of the previous tile is through with the stem tile
        if (tile + gridDim.x < n_tiles) fetch(tile + gridDim.x);
        __builtin_amdgcn_sched_barrier(0);                   // (the groups below count the LDS reads of the main loop only)

        // ---- 2. the stem outputs
        f32x16 acc[T::NTW];
#pragma unroll
        for (int ti = 0; ti < T::NTW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ti][r] = 0.f;
        // slots 2 j and 2 j + 1 are (kh, pw) = (j >> 1, 2 (j & 1) + hh); the fragments of step j + 1 are read while step j multiplies
        bf16x8 af[2][T::NTW];
#pragma unroll
        for (int ti = 0; ti < T::NTW; ++ti) af[0][ti] = *reinterpret_cast<const bf16x8*>(win + abase[ti]);
#pragma unroll
        for (int j = 0; j < 14; ++j) {
            const unsigned off = (unsigned)((((j + 1) >> 1) * T::WP + 2 * ((j + 1) & 1)) * 16);
#pragma unroll
            for (int ti = 0; ti < T::NTW; ++ti) {
                if (j < 13) af[(j + 1) & 1][ti] = *reinterpret_cast<const bf16x8*>(win + abase[ti] + off);
                acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[j], af[j & 1][ti], acc[ti], 0, 0, 0);
            }
        }
        // keep that order: one LDS read behind every MFMA (left alone, the scheduler sinks each read to just before its MFMA and the
        // wave waits out an LDS latency per MFMA)
        __builtin_amdgcn_sched_group_barrier(0x100, T::NTW, 0);  // the DS reads of step 0
#pragma unroll
        for (int k = 0; k < 13 * T::NTW; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        }
        __builtin_amdgcn_sched_group_barrier(0x008, T::NTW, 0);
        // (the accumulators are pinned here: otherwise the compiler sinks each tile's whole MFMA chain into the conditional block of
        // its epilogue below -- six serial chains of dependent MFMAs, each waiting for its own LDS read)
#pragma unroll
        for (int ti = 0; ti < T::NTW; ++ti) asm volatile("" : "+v"(acc[ti]));

        // ---- 3. shift, bf16, ReLU; the two swaps leave lanes 0-31 with channels 16 j .. 16 j + 7 of their pixel and lanes 32-63 with
        // channels 16 j + 8 .. 16 j + 15 (j = 0: pk[0..3], j = 1: pk[4..7])
#pragma unroll
        for (int ti = 0; ti < T::NTW; ++ti) {
            if ((tw + 2 * ti) * 32 < T::NPIX) {
                unsigned pk[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) pk[k] = relu_bf16x2(pack_bf16x2(acc[ti][2 * k] + sh[2 * k], acc[ti][2 * k + 1] + sh[2 * k + 1]));
                swap_halves(pk[0], pk[2]); swap_halves(pk[1], pk[3]);
                swap_halves(pk[4], pk[6]); swap_halves(pk[5], pk[7]);
                const int pi = (tw + 2 * ti) * 32 + l31;
                if (pi < T::NPIX) {
                    unsigned char* d = til + (unsigned)pi * T::ROW + (unsigned)((ct * 32 + 8 * hh) * 2);
                    *reinterpret_cast<uint4*>(d) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                    *reinterpret_cast<uint4*>(d + 32) = make_uint4(pk[4], pk[5], pk[6], pk[7]);
                }
            }
        }
        __syncthreads();             // the stem tile is there; every wave is through with the window

        // ---- 4. pool: one thread per (pooled pixel, 4 channels); tap (kh, kw) of local pooled (pp, qq) is local stem pixel
        // (2 pp + kh, 2 qq + kw) = stem pixel (2 (p0 + pp) - 1 + kh, 2 (q0 + qq) - 1 + kw).
        // The values went through the ReLU: no sign bit, so they order like their 16-bit patterns, every NaN above every number.  A window
        // that lies inside the stem map takes the maximum of the integer keys (value << 16) | (15 - tap): the greatest value, and among
        // equal values the first tap in scan order -- the scan rule of pool.hip without its three compares and two selects per element
        // and tap, which made this phase longer than everything before it (65 of 118 us).  A window that hangs over the edge of the map
        // or holds a NaN (the key says so) is scanned again by the rule as pool.hip writes it.
        for (int i = tid; i < TP * TQ * 16; i += 256) {
            const int c4 = i & 15, pq = i >> 4;
            const int pp = pq / TQ, qq = pq - pp * TQ;
            const int op = p0 + pp, oq = q0 + qq;
            if (op >= p.PP || oq >= p.PQ) continue;
            const unsigned char* w0 = til + (unsigned)(2 * pp * T::SW + 2 * qq) * T::ROW + (unsigned)c4 * 8u;
            unsigned key[4] = {0u, 0u, 0u, 0u};
    #pragma unroll
            for (int t = 0; t < 9; ++t) {
                const uint2 w = *reinterpret_cast<const uint2*>(w0 + (unsigned)((t / 3) * T::SW + t % 3) * T::ROW);
                const unsigned c = 15u - (unsigned)t;
                key[0] = max(key[0], (w.x << 16) | c);
                key[1] = max(key[1], (w.x & 0xffff0000u) | c);
                key[2] = max(key[2], (w.y << 16) | c);
                key[3] = max(key[3], (w.y & 0xffff0000u) | c);
            }
            uint2 yv;
            unsigned tv;
            yv.x = (key[0] >> 16) | (key[1] & 0xffff0000u);
            yv.y = (key[2] >> 16) | (key[3] & 0xffff0000u);
            tv = 0x0f0f0f0fu - ((key[0] & 15u) | ((key[1] & 15u) << 8) | ((key[2] & 15u) << 16) | ((key[3] & 15u) << 24));
            const bool inside = op > 0 && oq > 0 && 2 * op + 1 < p.P && 2 * oq + 1 < p.Q;
            if (!inside || max(max(key[0], key[1]), max(key[2], key[3])) > 0x7f80ffffu) {
                float best[4];
                unsigned bi[4];
    #pragma unroll
                for (int e = 0; e < 4; ++e) { best[e] = -INFINITY; bi[e] = 0u; }
                bool first = true;
    #pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int sy = 2 * op - 1 + kh;
                    if (sy < 0 || sy >= p.P) continue;
    #pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int sx = 2 * oq - 1 + kw;
                        if (sx < 0 || sx >= p.Q) continue;
                        const uint2 w = *reinterpret_cast<const uint2*>(w0 + (unsigned)(kh * T::SW + kw) * T::ROW);
                        const float v[4] = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                                            __uint_as_float(w.y & 0xffff0000u)};
    #pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            // ATen rule: take if strictly greater (or NaN); the first valid tap seeds the max
                            if (first || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = (unsigned)(kh * 3 + kw); }
                        }
                        first = false;
                    }
                }
                yv.x = pack_bf16x2(best[0], best[1]);
                yv.y = pack_bf16x2(best[2], best[3]);
                tv = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
            }
            const size_t o = ((n * (size_t)p.PP + (size_t)op) * (size_t)p.PQ + (size_t)oq) * 64u + (size_t)c4 * 4u;
            *reinterpret_cast<uint2*>(p.y + o) = yv;
            if (p.amax) *reinterpret_cast<unsigned*>(p.amax + o) = tv;
        }
    }
}

// pooled extents and the tile grid of an image; false = not served.  Image bases are 64-bit; what stays 32-bit is an offset inside one
// image and the workgroup count
struct SpShape {
    int Wh, P, Q, PP, PQ;
    unsigned tiles_x, tiles_y, grid;
};
bool sp_shape(int N, int H, int W, int K, SpShape& s) {
    if (K != 64 || N <= 0 || H < 7 || W < 7) return false;
    s.Wh = (W + 1) / 2;
    s.P = (H - 1) / 2 + 1; s.Q = (W - 1) / 2 + 1;
    s.PP = (s.P - 1) / 2 + 1; s.PQ = (s.Q - 1) / 2 + 1;
    if ((long long)H * s.Wh * 16 >= (1ll << 31) || (long long)s.PP * s.PQ * 128 >= (1ll << 31)) return false;
    s.tiles_x = (unsigned)cs_ceil_div(s.PQ, CS_STEM_POOL_TQ);
    s.tiles_y = (unsigned)cs_ceil_div(s.PP, CS_STEM_POOL_TP);
    const long long grid = (long long)N * s.tiles_x * s.tiles_y;
    if (grid >= (1ll << 31)) return false;
    s.grid = (unsigned)grid;
    return true;
}

}  // namespace

extern "C" int cs_stem_pool_fwd_supported(int N, int H, int W, int K) {
    SpShape s;
    return sp_shape(N, H, W, K, s) ? 1 : 0;
}

extern "C" int cs_stem_pool_fwd(int N, int H, int W, int K, const void* x_pair, const void* w_pair, const float* shift, void* y_pool,
                                uint8_t* argmax, void* stream) {
    CS_CHECK_ARG(x_pair && w_pair && y_pool, "stem_pool_fwd: x_pair, w_pair and y_pool must not be NULL");
    CS_CHECK_ARG(K == 64, "stem_pool_fwd: 64 output channels (the stem of every ResNet / ResNeXt of model/resnet.py)");
    SpShape s;
    CS_CHECK_ARG(sp_shape(N, H, W, K, s), "stem_pool_fwd: extents out of range (cs_stem_pool_fwd_supported)");
    using T = SpTile<CS_STEM_POOL_TP, CS_STEM_POOL_TQ>;
    auto fn = stem_pool_fwd_kernel<CS_STEM_POOL_TP, CS_STEM_POOL_TQ>;
    SpParams p;
    p.x = reinterpret_cast<const uint4*>(x_pair); p.w = reinterpret_cast<const uint4*>(w_pair); p.shift = shift;
    p.y = reinterpret_cast<bf16_t*>(y_pool); p.amax = argmax;
    p.H = H; p.Wh = s.Wh; p.P = s.P; p.Q = s.Q; p.PP = s.PP; p.PQ = s.PQ;
    p.N = (unsigned)N; p.tiles_x = s.tiles_x; p.tiles_y = s.tiles_y;
    if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(fn), T::LDS, 81920)) return CS_ERR_LAUNCH;
    char name[64];
    snprintf(name, sizeof(name), "stem_pool_fwd_kernel<%d,%d>", CS_STEM_POOL_TP, CS_STEM_POOL_TQ);
    cs_set_variant_(name);
    // persistent workgroups, two per compute unit (LDS and registers allow no third)
    const unsigned grid = std::min(s.grid, 2u * (unsigned)cs_device_cus_());
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), T::LDS, reinterpret_cast<hipStream_t>(stream), p);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
