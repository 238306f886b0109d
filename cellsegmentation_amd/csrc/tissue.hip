// Tissue detection for whole-slide streaming (tissue.py is the public API): which patches of a slide hold tissue at all, decided on
// the device before any of them costs two forwards of the network.  Four launches, all integer:
//   histogram  256 bins of the pixel feature f(r, g, b) per image.  A slide is mostly glass, so most pixels fall into the same few
//              bins: a thread counts RUNS of equal values in registers -- the run is carried across its whole stride, so a constant
//              image costs it one LDS atomic in all -- and only a change of value goes to one of the kCopies sub-histograms of
//              cs_pixels.h (a stride of 257 words puts one bin of the 16 copies into 16 banks; thread b folds bin b).
//   mask       f > thr[n] as 0 / 1, thr read from the device; the feature itself is never stored.
//   coverage   non-zero mask pixels under every patch: one workgroup per patch, a wave per row, dwords where the row is aligned.
//   select     order-preserving compaction of the patches with enough tissue: one workgroup, block_rank and a running base.
// The two pixel passes walk the images by cs_pixels.h (runs of 16 pixels as three 16-byte loads, single pixels on either side; no
// alignment is asked of the images or the mask).  Their grids are capped and stride over the image; every result is a sum or a
// comparison of integers, so neither the cap nor the order of arrival shows in it.
#include "cs_common.h"
#include "cs_block.h"
#include "cs_pixels.h"

namespace {

constexpr int kThreads = 256;                      // also the number of bins: thread b folds bin b
constexpr int kCopies = 16;                        // sub-histograms per workgroup
constexpr int kCopyStride = 257;                   // words between two copies: bin v of copy c in bank (c + v) mod 32
constexpr int kMaxTileBlocks = 1 << 16;            // of the coverage pass

template <int CH>
__device__ __forceinline__ int feature(int r, int g, int b) {
    if (CH == CS_TISSUE_CHROMA) return max(r, max(g, b)) - min(r, min(g, b));
    return 255 - ((77 * r + 150 * g + 29 * b + 128) >> 8);
}
template <int CH>
__device__ __forceinline__ int feature_at(const uint8_t* __restrict__ px, long long i) {
    return feature<CH>(px[3 * i], px[3 * i + 1], px[3 * i + 2]);
}

// the feature of pixel i of a run's words
template <int CH>
__device__ __forceinline__ int feature_of(const uint32_t (&w)[12], int i) {
    return feature<CH>(byte_of(w, 3 * i), byte_of(w, 3 * i + 1), byte_of(w, 3 * i + 2));
}

// A thread's run of equal values: `run` pixels of value `cur` not yet in its sub-histogram `mine` (an image has fewer than 2^31).
// A plain record that the walker's callbacks share: as a lambda inside those lambdas its two counters were left in scratch.
struct ValueRun {
    uint32_t* mine;
    int cur;
    uint32_t run;
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(mine + cur, run);
    }
    __device__ __forceinline__ void take(int v) {
        if (v == cur) {
            ++run;
        } else {
            flush();
            cur = v;
            run = 1;
        }
    }
};

// grid (blocks per image, N)
template <int CH>
__global__ __launch_bounds__(kThreads) void tissue_histogram_kernel(const uint8_t* __restrict__ images, long long HW,
                                                                    unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_hist[kCopies * kCopyStride];
    const int n = blockIdx.y;
    hist_zero<kThreads>(s_hist, kCopies, kCopyStride);
    __syncthreads();
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    ValueRun v{hist_mine(s_hist, kCopies, kCopyStride), 0, 0};
    for_pixels<kThreads>(
        s,
        [&](long long, const uint32_t(&w)[12]) {
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) v.take(feature_of<CH>(w, i));
        },
        [&](long long i) { v.take(feature_at<CH>(s.px, i)); });
    v.flush();
    hist_flush<kThreads>(s_hist, kCopies, kCopyStride, hist + (long long)n * 256);
}

// grid (blocks per image, N)
template <int CH>
__global__ __launch_bounds__(kThreads) void tissue_mask_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ thr,
                                                               uint8_t* __restrict__ mask) {
    const int n = blockIdx.y;
    const int t = thr[n];
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    uint8_t* out = mask + (long long)n * HW;
    const int width = access_width(out + s.head);
    for_pixels<kThreads>(
        s,
        [&](long long g, const uint32_t(&w)[12]) {
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) o[i >> 2] |= (uint32_t)(feature_of<CH>(w, i) > t) << (8 * (i & 3));
            store_words(out + s.head + kPixelRun * g, width, o);
        },
        [&](long long i) { out[i] = feature_at<CH>(s.px, i) > t; });
}

// the non-zero bytes of a dword
__device__ __forceinline__ int nonzero_bytes(uint32_t w) { return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u); }

// grid (min(T, kMaxTileBlocks)): a workgroup per patch, wave w its rows w, w + 4, ...; the window is clamped to the image
__global__ __launch_bounds__(kThreads) void tissue_coverage_kernel(const uint8_t* __restrict__ mask, int N, int H, int W,
                                                                   const int32_t* __restrict__ tile_img, const int32_t* __restrict__ tile_rc,
                                                                   long long T, int ph, int pw, int32_t* __restrict__ cover) {
    __shared__ int s_sum[kThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (long long t = blockIdx.x; t < T; t += gridDim.x) {                  // uniform: every thread reaches the barriers
        const int n = tile_img[t];
        const long long r = tile_rc[2 * t], c = tile_rc[2 * t + 1];
        const long long r0 = min(max(r, 0LL), (long long)H), r1 = min(max(r + ph, 0LL), (long long)H);
        const long long c0 = min(max(c, 0LL), (long long)W), c1 = min(max(c + pw, 0LL), (long long)W);
        int cnt = 0;
        if (n >= 0 && n < N && c1 > c0) {
            const int len = (int)(c1 - c0);
            for (long long row = r0 + wv; row < r1; row += kThreads / 64) {
                const uint8_t* p = mask + ((long long)n * H + row) * W + c0;
                const int head = min((int)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3), len);
                const int words = (len - head) >> 2, tail_at = head + 4 * words;
                for (int j = lane; j < words; j += 64) cnt += nonzero_bytes(*reinterpret_cast<const uint32_t*>(p + head + 4 * j));
                if (lane < head) cnt += p[lane] != 0;
                if (lane < len - tail_at) cnt += p[tail_at + lane] != 0;
            }
        }
        const int all = block_reduce<kThreads, int>(cnt, [](int a, int b) { return a + b; }, s_sum);
        if (threadIdx.x == 0) cover[t] = all;
    }
}

// grid (1)
__global__ __launch_bounds__(kThreads) void tissue_select_kernel(const int32_t* __restrict__ cover, long long T, int min_pixels,
                                                                 int32_t* __restrict__ selected, int32_t* __restrict__ n_selected) {
    __shared__ int s_wsum[kThreads / 64];
    long long base = 0;
    for (long long t0 = 0; t0 < T; t0 += kThreads) {
        const long long t = t0 + threadIdx.x;
        const bool keep = t < T && cover[t] >= min_pixels;
        int total;
        const int rank = block_rank<kThreads>(keep, s_wsum, total);
        if (keep) selected[base + rank] = (int32_t)t;
        base += total;
    }
    for (long long i = base + threadIdx.x; i < T; i += kThreads) selected[i] = -1;
    if (threadIdx.x == 0) n_selected[0] = (int32_t)base;
}

}  // namespace

extern "C" int cs_tissue_histogram(const uint8_t* images_hwc, int N, int H, int W, int channel, int64_t* hist, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "tissue_histogram: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(channel == CS_TISSUE_CHROMA || channel == CS_TISSUE_DARKNESS, "tissue_histogram: unknown channel");
    CS_CHECK_ARG(images_hwc && hist, "tissue_histogram: NULL argument");
    CS_CHECK_ARG(aligned(hist, 8), "tissue_histogram: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    if (channel == CS_TISSUE_CHROMA) hipLaunchKernelGGL(tissue_histogram_kernel<CS_TISSUE_CHROMA>, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, st, images_hwc, HW, h);
    else hipLaunchKernelGGL(tissue_histogram_kernel<CS_TISSUE_DARKNESS>, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, st, images_hwc, HW, h);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_tissue_mask(const uint8_t* images_hwc, int N, int H, int W, int channel, const int32_t* thr, uint8_t* mask, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "tissue_mask: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(channel == CS_TISSUE_CHROMA || channel == CS_TISSUE_DARKNESS, "tissue_mask: unknown channel");
    CS_CHECK_ARG(images_hwc && thr && mask, "tissue_mask: NULL argument");
    CS_CHECK_ARG(aligned(thr, 4), "tissue_mask: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W;
    if (channel == CS_TISSUE_CHROMA) hipLaunchKernelGGL(tissue_mask_kernel<CS_TISSUE_CHROMA>, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, st, images_hwc, HW, thr, mask);
    else hipLaunchKernelGGL(tissue_mask_kernel<CS_TISSUE_DARKNESS>, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, st, images_hwc, HW, thr, mask);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_tissue_coverage(const uint8_t* mask, int N, int H, int W, const int32_t* tile_img, const int32_t* tile_rc, long long T, int ph,
                                  int pw, int32_t* cover, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "tissue_coverage: need 0 < N <= 65535 masks of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(T >= 0 && T < (1LL << 31) && ph > 0 && pw > 0, "tissue_coverage: need 0 <= T < 2^31 windows of ph, pw > 0");
    CS_CHECK_ARG(mask && ((tile_img && tile_rc && cover) || T == 0), "tissue_coverage: NULL argument");
    CS_CHECK_ARG(aligned(tile_img, 4) && aligned(tile_rc, 4) && aligned(cover, 4), "tissue_coverage: misaligned argument");
    if (T == 0) return CS_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tissue_coverage_kernel, dim3((unsigned)(T < kMaxTileBlocks ? T : kMaxTileBlocks)), dim3(kThreads), 0, st, mask, N, H, W,
                       tile_img, tile_rc, T, ph, pw, cover);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_tissue_select(const int32_t* cover, long long T, int min_pixels, int32_t* selected, int32_t* n_selected, void* stream) {
    CS_CHECK_ARG(T >= 0 && T < (1LL << 31), "tissue_select: need 0 <= T < 2^31");
    CS_CHECK_ARG(n_selected && ((cover && selected) || T == 0), "tissue_select: NULL argument");
    CS_CHECK_ARG(aligned(cover, 4) && aligned(selected, 4) && aligned(n_selected, 4), "tissue_select: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tissue_select_kernel, dim3(1), dim3(kThreads), 0, st, cover, T, min_pixels, selected, n_selected);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
