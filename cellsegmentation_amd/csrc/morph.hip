// Nearest-site transform of N images [N][H][W] and what is built on it: exact disk morphology of masks and label expansion.
//   site      a pixel selected by a predicate on the input: uint8 != 0, uint8 == 0, or int32 != 0
//   rule      every pixel gets THE NEAREST SITE, AND AMONG EQUALLY NEAR SITES THE ONE WITH THE LOWEST ROW-MAJOR INDEX, i.e. the
//             smallest key (d2, site_row W + site_col) compared lexicographically; d2 is the exact squared Euclidean distance
//   columns   one thread per column: for every pixel the vertical distance g to the nearest site of its column and that site's row;
//             of a site above and a site below that are equally far, the one above is kept.  H < 46341, so g (0xffff = none) and
//             the row each fit 16 bits: one packed int32 of workspace per pixel
//   rows      one workgroup per row, the row's packed words in LDS: every pixel searches outwards over x +- d for the smallest key
//             (d^2 + g^2, site_row W + x +- d).  One site per column is enough: the kept one has the smallest g of its column and,
//             among those, the lowest row.  The search for a SITE runs while d^2 <= best: at d^2 == best a site on the pixel's own row
//             ties with the best so far and wins when that lies on a lower row -- offsets (3, 4) and (0, 5).  A search for the
//             distance alone may stop at d^2 >= best
//   bounded   morphology and label expansion only ask whether the nearest site lies within r2: their search stops at
//             d <= floor(sqrt(r2)), O(r) per pixel whatever the image holds.  Only the unbounded transform keeps the data-dependent
//             search (worst case: sparse sites in a wide image)
//   outside   the forms that need no site may count the pixels beyond the image edge as sites: the column sweeps start from
//             y + 1 / H - y and the row search also takes (x + 1)^2 and (W - x)^2
//   no site   an image without any site (and without the outside flag): d2 = -1 and site = -1 everywhere; no pixel is dilated, no
//             pixel is eroded, no label expands
// Integer work only; launches fixed by the shape; the one atomic is the OR into the per-image "has a site" flag, as in the EDT of
// detect.hip, whose column-sweep / row-search scheme this follows.
#include "cs_common.h"

namespace {

constexpr uint32_t kNoG = 0xffff;             // g of a column without a site
constexpr int kSiteLdsBytes = 160 * 1024;     // a row of packed words: W <= 40960
constexpr int kMaxSiteW = kSiteLdsBytes / 4;

enum { kSrcNonzero = 0, kSrcZero = 1, kSrcLabel = 2 };

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

__global__ __launch_bounds__(256) void morph_init_kernel(int32_t* __restrict__ has, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) has[i] = 0;
}

template <int SRC> __device__ __forceinline__ bool is_site(const void* src, long long off) {
    if (SRC == kSrcLabel) return reinterpret_cast<const int32_t*>(src)[off] != 0;
    const uint8_t v = reinterpret_cast<const uint8_t*>(src)[off];
    return SRC == kSrcZero ? v == 0 : v != 0;
}

// One thread per column (a wave reads 64 adjacent pixels of a row).  packed[y][x] = g << 16 | site_row: sweep down (nearest site at
// or above), then up over what the sweep down wrote; the site below replaces the one above only when it is strictly nearer.
// With `outside` rows -1 and H count as sites (their row number is never read: those forms take no site).
template <int SRC>
__global__ __launch_bounds__(64) void morph_column_kernel(const void* __restrict__ src, int H, int W, int outside,
                                                          uint32_t* __restrict__ packed, int32_t* __restrict__ has) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const long long img = (long long)blockIdx.y * H * W;
    bool seen = false;
    if (x < W) {
        uint32_t* col = packed + img + x;
        uint32_t d = outside ? 0 : kNoG;
#pragma unroll 8
        for (int y = 0; y < H; ++y) {
            const bool s = is_site<SRC>(src, img + (long long)y * W + x);
            seen |= s;
            d = s ? 0 : (d == kNoG ? kNoG : d + 1);
            col[(long long)y * W] = (d << 16) | ((uint32_t)(y - (int)d) & 0xffffu);
        }
        uint32_t u = outside ? 0 : kNoG;
#pragma unroll 8
        for (int y = H - 1; y >= 0; --y) {
            const uint32_t down = col[(long long)y * W] >> 16;
            u = down == 0 ? 0 : (u == kNoG ? kNoG : u + 1);
            if (u < down) col[(long long)y * W] = (u << 16) | ((uint32_t)(y + (int)u) & 0xffffu);
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

// ---- row pass, no site wanted: 16-bit g in LDS; out = erode ? d2 > r2 : d2 <= r2 ------------------------------------------------
// Dilation: sites are the nonzero pixels.  Erosion: sites are the zero pixels, and in && d2 > r2 is d2 > r2 (a zero pixel has d2 = 0).
// The search ends as soon as a site within r2 is found.  Without any site d2 is infinite: nothing is dilated, nothing eroded.
__global__ __launch_bounds__(256) void morph_binary_kernel(const uint32_t* __restrict__ packed, int H, int W, int outside,
                                                           const int32_t* __restrict__ has, int r2, int dlim, int erode,
                                                           uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];
    uint16_t* grow = reinterpret_cast<uint16_t*>(morph_lds);
    const long long base = ((long long)blockIdx.y * H + blockIdx.x) * W;
    if (!outside && !has[blockIdx.y]) {
        for (int x = threadIdx.x; x < W; x += blockDim.x) out[base + x] = (uint8_t)(erode != 0);
        return;
    }
    for (int x = threadIdx.x; x < W; x += blockDim.x) grow[x] = (uint16_t)(packed[base + x] >> 16);
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int g0 = grow[x];
        int best = g0 == (int)kNoG ? 0x7fffffff : g0 * g0;
        if (outside) best = min(best, min((x + 1) * (x + 1), (W - x) * (W - x)));
        const int dmax = min(dlim, max(x, W - 1 - x));
        for (int d = 1; d <= dmax && best > r2; ++d) {
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
        out[base + x] = (uint8_t)(erode ? best > r2 : best <= r2);
    }
}

// floor(sqrt(r2)) in integers
int isqrt_floor(int r2) {
    long long d = 0;
    while ((d + 1) * (d + 1) <= (long long)r2) ++d;
    return (int)d;
}

template <int SRC>
void launch_columns(const void* src, int N, int H, int W, int outside, uint32_t* packed, int32_t* has, hipStream_t s) {
    hipLaunchKernelGGL(morph_column_kernel<SRC>, dim3(cs_ceil_div(W, 64), N), dim3(64), 0, s, src, H, W, outside, packed, has);
}

// has-site flags cleared, then the column pass of `src_kind`
int columns(const void* src, int src_kind, int N, int H, int W, int outside, void* workspace, hipStream_t s) {
    int32_t* has = reinterpret_cast<int32_t*>(workspace);
    uint32_t* packed = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(workspace) + align16((size_t)N * 4));
    hipLaunchKernelGGL(morph_init_kernel, dim3(cs_ceil_div(N, 256)), dim3(256), 0, s, has, N);
    CS_LAUNCH_CHECK();
    if (src_kind == kSrcNonzero) launch_columns<kSrcNonzero>(src, N, H, W, outside, packed, has, s);
    else if (src_kind == kSrcZero) launch_columns<kSrcZero>(src, N, H, W, outside, packed, has, s);
    else launch_columns<kSrcLabel>(src, N, H, W, outside, packed, has, s);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

inline int row_threads(int W) { return W >= 256 ? 256 : cs_ceil_div(W, 64) * 64; }
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int cs_morph_max_site_width(void) { return kMaxSiteW; }

// workspace: has-site flag (int32 N), then one packed int32 per pixel
extern "C" size_t cs_morph_workspace(int N, int H, int W) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || (long long)H * H + (long long)W * W >= (1LL << 31)) return 0;
    return align16((size_t)N * 4) + align16((size_t)N * H * W * 4);
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
    const int rc = columns(src, src_is_labels ? kSrcLabel : (background ? kSrcZero : kSrcNonzero), N, H, W, 0, workspace, s);
    if (rc != CS_OK) return rc;
    const size_t lds = align16((size_t)W * 4);
    if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(morph_nearest_kernel), lds, kSiteLdsBytes)) return CS_ERR_LAUNCH;
    const int32_t* has = reinterpret_cast<const int32_t*>(workspace);
    const uint32_t* packed = reinterpret_cast<const uint32_t*>(reinterpret_cast<unsigned char*>(workspace) + align16((size_t)N * 4));
    hipLaunchKernelGGL(morph_nearest_kernel, dim3(H, N), dim3(row_threads(W)), lds, s, packed, H, W, has, d2, site);
    CS_LAUNCH_CHECK();
    return CS_OK;
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
    const int rc = columns(mask, erode ? kSrcZero : kSrcNonzero, N, H, W, outside_is_site != 0, workspace, s);
    if (rc != CS_OK) return rc;
    const size_t lds = align16((size_t)W * 2);
    if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(morph_binary_kernel), lds, 96 * 1024)) return CS_ERR_LAUNCH;
    const int32_t* has = reinterpret_cast<const int32_t*>(workspace);
    const uint32_t* packed = reinterpret_cast<const uint32_t*>(reinterpret_cast<unsigned char*>(workspace) + align16((size_t)N * 4));
    hipLaunchKernelGGL(morph_binary_kernel, dim3(H, N), dim3(row_threads(W)), lds, s, packed, H, W, (int)(outside_is_site != 0), has, r2,
                       isqrt_floor(r2), (int)(erode != 0), out);
    CS_LAUNCH_CHECK();
    return CS_OK;
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
    const int rc = columns(labels, kSrcLabel, N, H, W, 0, workspace, s);
    if (rc != CS_OK) return rc;
    const size_t lds = align16((size_t)W * 4);
    if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(morph_expand_kernel), lds, kSiteLdsBytes)) return CS_ERR_LAUNCH;
    const int32_t* has = reinterpret_cast<const int32_t*>(workspace);
    const uint32_t* packed = reinterpret_cast<const uint32_t*>(reinterpret_cast<unsigned char*>(workspace) + align16((size_t)N * 4));
    hipLaunchKernelGGL(morph_expand_kernel, dim3(H, N), dim3(row_threads(W)), lds, s, packed, labels, H, W, has, r2, isqrt_floor(r2), out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
