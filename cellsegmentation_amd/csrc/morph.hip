// Nearest-site transform of N images [N][H][W] and what is built on it: the exact Euclidean distance transform of
// method="distancetransform" (cs_detect_edt_*), exact disk morphology of masks and label expansion (cs_morph_*).
//   site      a pixel selected by a predicate on the input: uint8 != 0, uint8 == 0, int32 != 0, or, for the distance transform, whose
//             foreground is u8 > thr and whose sites are therefore the BACKGROUND pixels, uint8 <= thr and trunc(255 p) <= thr of fp32
//   rule      every pixel gets THE NEAREST SITE, AND AMONG EQUALLY NEAR SITES THE ONE WITH THE LOWEST ROW-MAJOR INDEX, i.e. the
//             smallest key (d2, site_row W + site_col) compared lexicographically; d2 is the exact squared Euclidean distance
//   columns   one thread per column: for every pixel the vertical distance g to the nearest site of its column and that site's row;
//             of a site above and a site below that are equally far, the one above is kept.  H < 46341, so g (0xffff = none) and
//             the row each fit 16 bits: one packed int32 per pixel (g << 16 | row; g alone where the row pass wants no site), in the
//             workspace or, for the distance transform, in the int32 output itself
//   rows      one workgroup per row, every pixel searching outwards over x +- d.  One site per column is enough: the kept one has the
//             smallest g of its column and, among those, the lowest row.
//             distance only: the row's 16-bit g in LDS (2 bytes per pixel: every admissible W), the smallest d^2 + g^2; the search
//             may stop at d^2 >= best.  The distance transform overwrites the row of g with d2 in place
//             site wanted: the row's packed words in LDS (4 bytes per pixel: W <= 40960), the smallest key
//             (d^2 + g^2, site_row W + x +- d).  This search runs while d^2 <= best: at d^2 == best a site on the pixel's own row
//             ties with the best so far and wins when that lies on a lower row -- offsets (3, 4) and (0, 5)
//   bounded   morphology and label expansion only ask whether the nearest site lies within r2: their search stops at
//             d <= floor(sqrt(r2)), O(r) per pixel whatever the image holds.  The unbounded forms keep the data-dependent search
//             (worst case: sparse sites in a wide image)
//   outside   the forms that need no site may count the pixels beyond the image edge as sites: the column sweeps start from
//             y + 1 / H - y and the row search also takes (x + 1)^2 and (W - x)^2
//   no site   an image without any site (and without the outside flag): d2 = -1 and site = -1 everywhere; no pixel is dilated, no
//             pixel is eroded, no label expands; the distance transform's maximum of the map stays -1
//   smoothed  per-map maximum M of d2 by integer atomicMax, one per row; 255 sqrt(d2 / M) rounded half to even, decided by
//             4 255^2 d2 <> (2k + 1)^2 M in int64
// Integer work only; launches fixed by the shape; the atomics are the OR into the per-image "has a site" flag and that maximum.
#include "cs_common.h"

namespace {

constexpr uint32_t kNoG = 0xffff;             // g of a column without a site
constexpr int kSiteLdsBytes = 160 * 1024;     // a row of packed words: W <= 40960
constexpr int kMaxSiteW = kSiteLdsBytes / 4;
constexpr int kGLdsBytes = 96 * 1024;         // a row of 16-bit g: every W below 46341

enum { kSrcNonzero = 0, kSrcZero = 1, kSrcLabel = 2, kSrcU8AtMost = 3, kSrcF32AtMost = 4 };

// has[0..N) = 0; map_max[0..N) = -1 where the caller keeps per-map maxima (NULL otherwise)
__global__ __launch_bounds__(256) void morph_init_kernel(int32_t* __restrict__ has, int32_t* __restrict__ map_max, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        has[i] = 0;
        if (map_max) map_max[i] = -1;
    }
}

// thr is read by the two "at most" kinds only
template <int SRC> __device__ __forceinline__ bool is_site(const void* src, long long off, int thr) {
    if (SRC == kSrcLabel) return reinterpret_cast<const int32_t*>(src)[off] != 0;
    if (SRC == kSrcF32AtMost) return (int)quant(reinterpret_cast<const float*>(src)[off]) <= thr;
    const uint8_t v = reinterpret_cast<const uint8_t*>(src)[off];
    if (SRC == kSrcU8AtMost) return (int)v <= thr;
    return SRC == kSrcZero ? v == 0 : v != 0;
}

// One thread per column (a wave reads 64 adjacent pixels of a row): sweep down (nearest site at or above), then up over what the sweep
// down wrote; the site below replaces the one above only when it is strictly nearer.  SITE: packed[y][x] = g << 16 | site_row;
// otherwise, for a row pass that reads g alone, packed[y][x] = g.  With `outside` rows -1 and H count as sites (SITE = false only).
// Both sweeps count g in the unit the word holds it in (kGOne), so that the word without a site row is g as it stands: a whole-slide
// mask gives every SIMD one wave at most, each walking its column row by row, and every instruction per row shows in the time
// (packing rows that the distance transform never reads cost it 4 % on a 4096^2 mask).
template <int SRC, bool SITE>
__global__ __launch_bounds__(64) void morph_column_kernel(const void* __restrict__ src, int H, int W, int thr, int outside,
                                                          uint32_t* __restrict__ packed, int32_t* __restrict__ has) {
    constexpr uint32_t kGOne = SITE ? 1u << 16 : 1u, kGNone = kNoG * kGOne;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const long long img = (long long)blockIdx.y * H * W;
    bool seen = false;
    if (x < W) {
        uint32_t* col = packed + img + x;
        uint32_t d = outside ? 0 : kGNone, above = 0;              // g in units of kGOne; the row of the nearest site at or above
#pragma unroll 8
        for (int y = 0; y < H; ++y) {
            const bool s = is_site<SRC>(src, img + (long long)y * W + x, thr);
            d = s ? 0 : (d == kGNone ? kGNone : d + kGOne);
            if (SITE) above = s ? (uint32_t)y : above;
            col[(long long)y * W] = SITE ? d | above : d;
        }
        seen = d != kGNone;                                        // once a site is met, d stays finite; the outside counts as one
        uint32_t u = outside ? 0 : kGNone, below = 0;
#pragma unroll 8
        for (int y = H - 1; y >= 0; --y) {
            const uint32_t word = col[(long long)y * W];
            const uint32_t down = SITE ? word & 0xffff0000u : word;
            u = down == 0 ? 0 : (u == kGNone ? kGNone : u + kGOne);
            if (SITE) below = down == 0 ? (uint32_t)y : below;
            if (u < down) col[(long long)y * W] = SITE ? u | below : u;
        }
    }
    if (__any(seen) && threadIdx.x == 0) atomicOr(has + blockIdx.y, 1);
}

// ---- row pass, site wanted: the smallest key (d2 << 32 | site) as one unsigned 64-bit minimum ------------------------------------
constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ unsigned long long site_key(uint32_t word, int dd, int W, int col) {
    const uint32_t g = word >> 16;
    if (g == kNoG) return kNoKey;
    return ((unsigned long long)(uint32_t)(dd + (int)(g * g)) << 32) | (uint32_t)((int)(word & 0xffffu) * W + col);
}

// dlim: the largest |dx| searched (W for the unbounded transform, floor(sqrt(r2)) for the expansion).
__device__ __forceinline__ unsigned long long nearest_key(const uint32_t* row, int W, int x, int dlim) {
    unsigned long long best = site_key(row[x], 0, W, x);
    const int dmax = min(dlim, max(x, W - 1 - x));
    for (int d = 1; d <= dmax && (unsigned long long)(d * d) <= (best >> 32); ++d) {
        const int dd = d * d;
        if (x - d >= 0) best = min(best, site_key(row[x - d], dd, W, x - d));
        if (x + d < W) best = min(best, site_key(row[x + d], dd, W, x + d));
    }
    return best;
}

__device__ __forceinline__ void stage_row(uint32_t* lds, const uint32_t* __restrict__ src, int W) {
    for (int x = threadIdx.x; x < W; x += blockDim.x) lds[x] = src[x];
    __syncthreads();
}

// d2 and / or site (either may be NULL), int32 [N][H][W]; site = flat index row W + col within the image
__global__ __launch_bounds__(256) void morph_nearest_kernel(const uint32_t* __restrict__ packed, int H, int W,
                                                            const int32_t* __restrict__ has, int32_t* __restrict__ d2,
                                                            int32_t* __restrict__ site) {
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];
    uint32_t* row = reinterpret_cast<uint32_t*>(morph_lds);
    const long long base = ((long long)blockIdx.y * H + blockIdx.x) * W;
    if (!has[blockIdx.y]) {
        for (int x = threadIdx.x; x < W; x += blockDim.x) {
            if (d2) d2[base + x] = -1;
            if (site) site[base + x] = -1;
        }
        return;
    }
    stage_row(row, packed + base, W);
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const unsigned long long k = nearest_key(row, W, x, W);
        if (d2) d2[base + x] = (int32_t)(k >> 32);
        if (site) site[base + x] = (int32_t)(uint32_t)k;
    }
}

// out = in != 0 ? in : (d2 <= r2 ? in[site] : 0).  A nonzero pixel is its own site at distance 0, so this is in[site] wherever
// d2 <= r2.  out must not overlap in.
__global__ __launch_bounds__(256) void morph_expand_kernel(const uint32_t* __restrict__ packed, const int32_t* __restrict__ in, int H,
                                                           int W, const int32_t* __restrict__ has, int r2, int dlim,
                                                           int32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];
    uint32_t* row = reinterpret_cast<uint32_t*>(morph_lds);
    const long long img = (long long)blockIdx.y * H * W;
    const long long base = img + (long long)blockIdx.x * W;
    if (!has[blockIdx.y]) {
        for (int x = threadIdx.x; x < W; x += blockDim.x) out[base + x] = 0;
        return;
    }
    stage_row(row, packed + base, W);
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const unsigned long long k = nearest_key(row, W, x, dlim);
        out[base + x] = (k >> 32) <= (unsigned long long)r2 ? in[img + (uint32_t)k] : 0;
    }
}

// ---- row pass, distance only: the row's g (words of a column pass without SITE) as 16-bit values in LDS ------------------------------
// Every global read of the row happens before the barrier, so a caller may afterwards overwrite the row it staged.
__device__ __forceinline__ void stage_g(uint16_t* grow, const uint32_t* packed_row, int W) {
    for (int x = threadIdx.x; x < W; x += blockDim.x) grow[x] = (uint16_t)packed_row[x];
    __syncthreads();
}

// min over x' of (x - x')^2 + g[x']^2 (0x7fffffff without a site in reach), with `outside` also over the columns beyond either edge.
// dlim: the largest |dx| searched; stop: the search also ends once best <= stop.  Every sum stays below H^2 + W^2 < 2^31.
// The loop runs while d <= dmax && d^2 < best && best > stop, and each of its two callers only ever sees the conditions it needs:
//   distance transform (dlim = W, stop = -1): best >= 0 > stop always holds, so the loop is d <= max(x, W - 1 - x) && d^2 < best;
//   morphology (dlim = floor(sqrt(r2)), stop = r2): d <= dlim and best > r2 give d^2 <= r2 < best, so d^2 < best never ends the
//   loop, which is d <= dmax && best > r2 -- it ends at the first site within r2.
// Not for a search that returns the site: that one has to go on through d^2 == best (nearest_key).
__device__ __forceinline__ int nearest_d2(const uint16_t* grow, int W, int x, int dlim, int stop, int outside) {
    const int g0 = grow[x];
    int best = g0 == (int)kNoG ? 0x7fffffff : g0 * g0;
    if (outside) best = min(best, min((x + 1) * (x + 1), (W - x) * (W - x)));
    const int dmax = min(dlim, max(x, W - 1 - x));
    for (int d = 1; d <= dmax && d * d < best && best > stop; ++d) {
        const int dd = d * d;
        if (x - d >= 0) {
            const int gl = grow[x - d];
            if (gl != (int)kNoG) best = min(best, dd + gl * gl);
        }
        if (x + d < W) {
            const int gr = grow[x + d];
            if (gr != (int)kNoG) best = min(best, dd + gr * gr);
        }
    }
    return best;
}

// out = erode ? d2 > r2 : d2 <= r2.  Dilation: sites are the nonzero pixels.  Erosion: sites are the zero pixels, and in && d2 > r2
// is d2 > r2 (a zero pixel has d2 = 0).  Without any site d2 is infinite: nothing is dilated, nothing eroded.
__global__ __launch_bounds__(256) void morph_binary_kernel(const uint32_t* __restrict__ packed, int H, int W, int outside,
                                                           const int32_t* __restrict__ has, int r2, int dlim, int erode,
                                                           uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];
    uint16_t* grow = reinterpret_cast<uint16_t*>(morph_lds);
    const long long base = ((long long)blockIdx.y * H + blockIdx.x) * W;
    if (!has[blockIdx.y]) {                                        // never with `outside`: the column pass counts it as a site
        for (int x = threadIdx.x; x < W; x += blockDim.x) out[base + x] = (uint8_t)(erode != 0);
        return;
    }
    stage_g(grow, packed + base, W);
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int best = nearest_d2(grow, W, x, dlim, r2, outside);
        out[base + x] = (uint8_t)(erode ? best > r2 : best <= r2);
    }
}

// The distance transform's row pass, in place: d2 holds the g of the column pass and leaves holding the squared distances.
// The row's maximum is reduced by shuffles and leaves by one atomicMax.  A map without a site gets -1 without being read; its
// maximum stays -1.
__global__ __launch_bounds__(256) void morph_d2_kernel(int32_t* __restrict__ d2, int H, int W, const int32_t* __restrict__ has,
                                                       int32_t* __restrict__ map_max) {
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];
    uint16_t* grow = reinterpret_cast<uint16_t*>(morph_lds);
    __shared__ int wmax[4];
    const int n = blockIdx.y;
    int32_t* row = d2 + ((long long)n * H + blockIdx.x) * W;
    if (!has[n]) {
        for (int x = threadIdx.x; x < W; x += blockDim.x) row[x] = -1;
        return;
    }
    stage_g(grow, reinterpret_cast<const uint32_t*>(row), W);
    int lmax = 0;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int best = nearest_d2(grow, W, x, W, -1, 0);
        row[x] = best;
        lmax = max(lmax, best);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lmax = max(lmax, __shfl_xor(lmax, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = lmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) lmax = max(lmax, wmax[w]);
        atomicMax(map_max + n, lmax);
    }
}

// 255 sqrt(D2 / M) rounded half to even: the float estimate is moved until (2k - 1)^2 M <= 4 255^2 D2 <= (2k + 1)^2 M holds in
// int64 (all products < 2^50); equality on either side is a tie between two integers and goes to the even one.
__device__ __forceinline__ uint8_t edt_norm(int32_t d2, int32_t M) {
    if (M <= 0 || d2 <= 0) return 0;
    const long long A = 4LL * 255 * 255 * d2;
    int k = (int)(255.0f * sqrtf((float)d2 / (float)M) + 0.5f);
    k = min(max(k, 0), 255);
    while (k > 0 && A < (long long)(2 * k - 1) * (2 * k - 1) * M) --k;
    while (A > (long long)(2 * k + 1) * (2 * k + 1) * M) ++k;
    if (A == (long long)(2 * k + 1) * (2 * k + 1) * M) return (uint8_t)((k & 1) ? k + 1 : k);
    if (k > 0 && A == (long long)(2 * k - 1) * (2 * k - 1) * M) return (uint8_t)((k & 1) ? k - 1 : k);
    return (uint8_t)k;
}

// four consecutive pixels of the flat [N H W] range per thread; a group may straddle maps (H W need not be a multiple of 4)
__global__ __launch_bounds__(256) void edt_normalise_kernel(const int32_t* __restrict__ d2, const int32_t* __restrict__ map_max, long long HW,
                                                            long long total, uint8_t* __restrict__ out) {
    const long long t4 = total >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < t4; i += (long long)gridDim.x * 256) {
        const int4 v = reinterpret_cast<const int4*>(d2)[i];
        long long n = (4 * i) / HW, rem = 4 * i - n * HW;
        const int32_t dv[4] = {v.x, v.y, v.z, v.w};
        uint32_t o = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            while (rem >= HW) {
                rem -= HW;
                ++n;
            }
            o |= (uint32_t)edt_norm(dv[q], map_max[n]) << (8 * q);
            ++rem;
        }
        reinterpret_cast<uint32_t*>(out)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (total & 3)) {
        const long long i = t4 * 4 + threadIdx.x;
        out[i] = edt_norm(d2[i], map_max[i / HW]);
    }
}

// floor(sqrt(r2)) in integers
int isqrt_floor(int r2) {
    long long d = 0;
    while ((d + 1) * (d + 1) <= (long long)r2) ++d;
    return (int)d;
}

inline bool dims_ok(int N, int H, int W) {
    return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * H + (long long)W * W < (1LL << 31);
}
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int SRC, bool SITE>
void launch_columns(const void* src, int N, int H, int W, int thr, int outside, uint32_t* packed, int32_t* has, hipStream_t s) {
    hipLaunchKernelGGL((morph_column_kernel<SRC, SITE>), dim3(cs_ceil_div(W, 64), N), dim3(64), 0, s, src, H, W, thr, outside, packed,
                       has);
}

// has-site flags cleared (and the per-map maxima, where map_max is given), then the column pass of `src_kind` into `packed`; `site`:
// the row pass wants the site's row, not g alone (the label kind always does, the two "at most" kinds never)
int columns(const void* src, int src_kind, int thr, bool site, int N, int H, int W, int outside, uint32_t* packed, int32_t* has,
            int32_t* map_max, hipStream_t s) {
    hipLaunchKernelGGL(morph_init_kernel, dim3(cs_ceil_div(N, 256)), dim3(256), 0, s, has, map_max, N);
    CS_LAUNCH_CHECK();
    if (src_kind == kSrcLabel) launch_columns<kSrcLabel, true>(src, N, H, W, thr, outside, packed, has, s);
    else if (src_kind == kSrcU8AtMost) launch_columns<kSrcU8AtMost, false>(src, N, H, W, thr, outside, packed, has, s);
    else if (src_kind == kSrcF32AtMost) launch_columns<kSrcF32AtMost, false>(src, N, H, W, thr, outside, packed, has, s);
    else if (src_kind == kSrcZero && site) launch_columns<kSrcZero, true>(src, N, H, W, thr, outside, packed, has, s);
    else if (src_kind == kSrcZero) launch_columns<kSrcZero, false>(src, N, H, W, thr, outside, packed, has, s);
    else if (site) launch_columns<kSrcNonzero, true>(src, N, H, W, thr, outside, packed, has, s);
    else launch_columns<kSrcNonzero, false>(src, N, H, W, thr, outside, packed, has, s);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

inline int row_threads(int W) { return W >= 256 ? 256 : cs_ceil_div(W, 64) * 64; }

// one workgroup per row with the row in dynamic LDS: 2 bytes per pixel (g alone) or 4 (packed words)
template <typename Kernel, typename... Args>
int launch_rows(Kernel kernel, int bytes_per_pixel, int N, int H, int W, hipStream_t s, Args... args) {
    const size_t lds = cs_align16((size_t)W * bytes_per_pixel);
    if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(kernel), lds, bytes_per_pixel == 2 ? kGLdsBytes : kSiteLdsBytes))
        return CS_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(H, N), dim3(row_threads(W)), lds, s, args...);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

// workspace of the cs_morph_* calls: has-site flag (int32 N), then one packed int32 per pixel
struct MorphScratch {
    int32_t* has;
    uint32_t* packed;
};
inline MorphScratch carve(void* workspace, int N) {
    return {reinterpret_cast<int32_t*>(workspace),
            reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(workspace) + cs_align16((size_t)N * 4))};
}

// st[0..N) = per-map maximum of d2, st[N..2N) = "the map has a background pixel"; d2 takes g, then the distances
int edt_sq_launch(const void* src, int src_is_f32, int N, int H, int W, int thr, int32_t* d2, int32_t* st, hipStream_t s) {
    const int rc = columns(src, src_is_f32 ? kSrcF32AtMost : kSrcU8AtMost, thr, false, N, H, W, 0, reinterpret_cast<uint32_t*>(d2), st + N, st, s);
    if (rc != CS_OK) return rc;
    return launch_rows(morph_d2_kernel, 2, N, H, W, s, d2, H, W, st + N, st);
}

}  // namespace

// workspace: st (int32 2 N: per-map maximum, has-background flag), then for the smoothed form D2 (int32 N H W)
extern "C" size_t cs_detect_edt_workspace(int N, int H, int W, int smooth) {
    if (!dims_ok(N, H, W)) return 0;
    return cs_align16((size_t)N * 8) + (smooth ? cs_align16((size_t)N * H * W * 4) : 0);
}

extern "C" int cs_detect_edt_sq(const void* src, int src_is_f32, int N, int H, int W, int thr, int32_t* d2, void* workspace,
                                size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(src && d2 && workspace, "detect_edt_sq: NULL argument");
    const size_t need = cs_detect_edt_workspace(N, H, W, 0);
    CS_CHECK_ARG(need > 0, "detect_edt_sq: needs 0 < N <= 65535 maps with H^2 + W^2 < 2^31");
    CS_CHECK_ARG(workspace_bytes >= need, "detect_edt_sq: workspace too small");
    CS_CHECK_ARG(aligned(workspace, 16) && aligned(d2, 4) && (!src_is_f32 || aligned(src, 4)), "detect_edt_sq: misaligned buffers");
    return edt_sq_launch(src, src_is_f32, N, H, W, thr, d2, reinterpret_cast<int32_t*>(workspace), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int cs_detect_edt_smooth(const void* src, int src_is_f32, int N, int H, int W, int thr, uint8_t* dst, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(src && dst && workspace, "detect_edt_smooth: NULL argument");
    const size_t need = cs_detect_edt_workspace(N, H, W, 1);
    CS_CHECK_ARG(need > 0, "detect_edt_smooth: needs 0 < N <= 65535 maps with H^2 + W^2 < 2^31");
    CS_CHECK_ARG(workspace_bytes >= need, "detect_edt_smooth: workspace too small");
    CS_CHECK_ARG(aligned(workspace, 16) && aligned(dst, 4) && (!src_is_f32 || aligned(src, 4)), "detect_edt_smooth: misaligned buffers");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int32_t* st = reinterpret_cast<int32_t*>(workspace);
    int32_t* d2 = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(workspace) + cs_align16((size_t)N * 8));
    const int rc = edt_sq_launch(src, src_is_f32, N, H, W, thr, d2, st, s);
    if (rc != CS_OK) return rc;
    // four pixels per thread, grid-stride over at most 8192 workgroups
    const long long HW = (long long)H * W, total = HW * N, blocks = ((total + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(edt_normalise_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, s, d2, st, HW, total, dst);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_morph_max_site_width(void) { return kMaxSiteW; }

extern "C" size_t cs_morph_workspace(int N, int H, int W) {
    if (!dims_ok(N, H, W)) return 0;
    return cs_align16((size_t)N * 4) + cs_align16((size_t)N * H * W * 4);
}

extern "C" int cs_morph_nearest(const void* src, int src_is_labels, int background, int N, int H, int W, int32_t* d2, int32_t* site,
                                void* workspace, size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(src && workspace && (d2 || site), "morph_nearest: NULL argument");
    CS_CHECK_ARG(!(src_is_labels && background), "morph_nearest: the background of a label image is not a site set");
    const size_t need = cs_morph_workspace(N, H, W);
    CS_CHECK_ARG(need > 0, "morph_nearest: needs 0 < N <= 65535 images with H^2 + W^2 < 2^31");
    CS_CHECK_ARG(W <= kMaxSiteW, "morph_nearest: rows wider than 40960 pixels do not fit the LDS");
    CS_CHECK_ARG(workspace_bytes >= need, "morph_nearest: workspace too small");
    CS_CHECK_ARG(aligned(workspace, 16) && aligned(d2, 4) && aligned(site, 4) && (!src_is_labels || aligned(src, 4)),
                 "morph_nearest: misaligned buffers");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MorphScratch w = carve(workspace, N);
    const int kind = src_is_labels ? kSrcLabel : (background ? kSrcZero : kSrcNonzero);
    const int rc = columns(src, kind, 0, true, N, H, W, 0, w.packed, w.has, nullptr, s);
    if (rc != CS_OK) return rc;
    return launch_rows(morph_nearest_kernel, 4, N, H, W, s, w.packed, H, W, w.has, d2, site);
}

extern "C" int cs_morph_binary(const uint8_t* mask, int N, int H, int W, int erode, int r2, int outside_is_site, uint8_t* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(mask && out && workspace, "morph_binary: NULL argument");
    CS_CHECK_ARG(r2 >= 0, "morph_binary: r2 must not be negative");
    const size_t need = cs_morph_workspace(N, H, W);
    CS_CHECK_ARG(need > 0, "morph_binary: needs 0 < N <= 65535 images with H^2 + W^2 < 2^31");
    CS_CHECK_ARG(workspace_bytes >= need, "morph_binary: workspace too small");
    CS_CHECK_ARG(aligned(workspace, 16), "morph_binary: misaligned buffers");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MorphScratch w = carve(workspace, N);
    const int outside = outside_is_site != 0;
    const int rc = columns(mask, erode ? kSrcZero : kSrcNonzero, 0, false, N, H, W, outside, w.packed, w.has, nullptr, s);
    if (rc != CS_OK) return rc;
    return launch_rows(morph_binary_kernel, 2, N, H, W, s, w.packed, H, W, outside, w.has, r2, isqrt_floor(r2), (int)(erode != 0), out);
}

extern "C" int cs_morph_expand_labels(const int32_t* labels, int N, int H, int W, int r2, int32_t* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(labels && out && workspace, "morph_expand_labels: NULL argument");
    CS_CHECK_ARG(labels != out, "morph_expand_labels: out must not be the input");
    CS_CHECK_ARG(r2 >= 0, "morph_expand_labels: r2 must not be negative");
    const size_t need = cs_morph_workspace(N, H, W);
    CS_CHECK_ARG(need > 0, "morph_expand_labels: needs 0 < N <= 65535 images with H^2 + W^2 < 2^31");
    CS_CHECK_ARG(W <= kMaxSiteW, "morph_expand_labels: rows wider than 40960 pixels do not fit the LDS");
    CS_CHECK_ARG(workspace_bytes >= need, "morph_expand_labels: workspace too small");
    CS_CHECK_ARG(aligned(workspace, 16) && aligned(labels, 4) && aligned(out, 4), "morph_expand_labels: misaligned buffers");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MorphScratch w = carve(workspace, N);
    const int rc = columns(labels, kSrcLabel, 0, true, N, H, W, 0, w.packed, w.has, nullptr, s);
    if (rc != CS_OK) return rc;
    return launch_rows(morph_expand_kernel, 4, N, H, W, s, w.packed, labels, H, W, w.has, r2, isqrt_floor(r2), out);
}
