// Tissue detection for whole-slide streaming (tissue.py is the public API): which patches of a slide hold tissue at all, decided on
// the device before any of them costs two forwards of the network.  Four launches, all integer:
//   histogram  256 bins of the pixel feature f(r, g, b) per image.  A slide is mostly glass, so most pixels fall into the same few
//              bins: a thread counts RUNS of equal values in registers -- the run is carried across its whole stride, so a constant
//              image costs it one LDS atomic in all -- and only a change of value goes to one of kCopies sub-histograms of the
//              workgroup (lane & 15 picks the copy; a stride of 257 words puts one bin of the 16 copies into 16 banks).  The
//              workgroup folds its copies, thread b owning bin b, and adds the non-zero sums with one 64-bit integer atomic each.
//   mask       f > thr[n] as 0 / 1, thr read from the device; the feature itself is never stored.
//   coverage   non-zero mask pixels under every patch: one workgroup per patch, a wave per row, dwords where the row is aligned.
//   select     order-preserving compaction of the patches with enough tissue: one workgroup, block_rank and a running base.
// The two pixel passes read 16 pixels = 48 bytes per thread and step as three 16-byte loads.  A pixel boundary that is also a
// 16-byte boundary exists within the first 16 pixels of any image (3 is invertible mod 16), so no alignment is asked of the images:
// the fewer than 16 pixels before it and the fewer than 16 after the last whole run are taken one by one by the image's first
// workgroup.  Grids are capped and stride over the image; every result is a sum or a comparison of integers, so neither the cap
// nor the order of arrival shows in it.
#include "cs_common.h"
#include "cs_block.h"

namespace {

constexpr int kThreads = 256;                      // also the number of bins: thread b folds bin b
constexpr int kRun = 16;                           // pixels per thread and step
constexpr int kCopies = 16;                        // sub-histograms per workgroup
constexpr int kCopyStride = 257;                   // words between two copies: bin v of copy c in bank (c + v) mod 32
constexpr int kMaxBlocks = 2048;                   // of one pixel pass, all images together (an image has at least one)
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

// image n as [0, head) single pixels, `runs` runs of kRun pixels from the 16-byte boundary at pixel `head` on, [tail_at, HW) singles
struct Span {
    const uint8_t* px;
    long long head, runs, tail_at, HW;
};
__device__ __forceinline__ Span image_span(const uint8_t* __restrict__ images, int n, long long HW) {
    Span s;
    s.px = images + (long long)n * HW * 3;
    s.HW = HW;
    // the smallest k with (px + 3 k) % 16 == 0: 3 * 11 = 33 = 1 (mod 16), so k = 11 * (-px) (mod 16)
    const long long k = (11 * ((16 - (int)(reinterpret_cast<uintptr_t>(s.px) & 15)) & 15)) & 15;
    s.head = k < HW ? k : HW;
    s.runs = (HW - s.head) / kRun;
    s.tail_at = s.head + s.runs * kRun;
    return s;
}

// the features of the 16 pixels in the 48 bytes at p (16-byte aligned)
template <int CH>
__device__ __forceinline__ void features16(const uint8_t* __restrict__ p, int (&f)[kRun]) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1], c = reinterpret_cast<const uint4*>(p)[2];
    const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
        const int o = 3 * i;
        f[i] = feature<CH>((w[o >> 2] >> (8 * (o & 3))) & 255, (w[(o + 1) >> 2] >> (8 * ((o + 1) & 3))) & 255,
                           (w[(o + 2) >> 2] >> (8 * ((o + 2) & 3))) & 255);
    }
}

// grid (blocks per image, N)
template <int CH>
__global__ __launch_bounds__(kThreads) void tissue_histogram_kernel(const uint8_t* __restrict__ images, long long HW,
                                                                    unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_hist[kCopies * kCopyStride];
    const int n = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kCopies * kCopyStride; i += kThreads) s_hist[i] = 0;
    __syncthreads();
    uint32_t* mine = s_hist + (tid & (kCopies - 1)) * kCopyStride;
    const Span s = image_span(images, n, HW);
    int cur = 0;
    uint32_t run = 0;                              // pixels of value cur not yet in LDS; an image has fewer than 2^31
    auto take = [&](int v) {
        if (v == cur) {
            ++run;
        } else {
            if (run) atomicAdd(mine + cur, run);
            cur = v;
            run = 1;
        }
    };
    for (long long g = (long long)blockIdx.x * kThreads + tid; g < s.runs; g += (long long)gridDim.x * kThreads) {
        int f[kRun];
        features16<CH>(s.px + 3 * (s.head + kRun * g), f);
#pragma unroll
        for (int i = 0; i < kRun; ++i) take(f[i]);
    }
    if (blockIdx.x == 0) {                         // fewer than kRun pixels on either side
        if (tid < s.head) take(feature_at<CH>(s.px, tid));
        if (tid < s.HW - s.tail_at) take(feature_at<CH>(s.px, s.tail_at + tid));
    }
    if (run) atomicAdd(mine + cur, run);
    __syncthreads();
    uint32_t sum = 0;                              // the workgroup's pixels: below 2^31 as well
#pragma unroll
    for (int c = 0; c < kCopies; ++c) sum += s_hist[c * kCopyStride + tid];
    if (sum) atomicAdd(hist + (long long)n * 256 + tid, (unsigned long long)sum);
}

// grid (blocks per image, N)
template <int CH>
__global__ __launch_bounds__(kThreads) void tissue_mask_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ thr,
                                                               uint8_t* __restrict__ mask) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const int t = thr[n];
    const Span s = image_span(images, n, HW);
    uint8_t* out = mask + (long long)n * HW;
    const uintptr_t at = reinterpret_cast<uintptr_t>(out + s.head);          // uniform: every run of the image starts 16 k bytes on
    const int align = (at & 15) == 0 ? 16 : (at & 3) == 0 ? 4 : 1;
    for (long long g = (long long)blockIdx.x * kThreads + tid; g < s.runs; g += (long long)gridDim.x * kThreads) {
        int f[kRun];
        features16<CH>(s.px + 3 * (s.head + kRun * g), f);
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kRun; ++i) o[i >> 2] |= (uint32_t)(f[i] > t) << (8 * (i & 3));
        uint8_t* q = out + s.head + kRun * g;
        if (align == 16) {
            *reinterpret_cast<uint4*>(q) = make_uint4(o[0], o[1], o[2], o[3]);
        } else if (align == 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) reinterpret_cast<uint32_t*>(q)[j] = o[j];
        } else {
#pragma unroll
            for (int i = 0; i < kRun; ++i) q[i] = (uint8_t)((o[i >> 2] >> (8 * (i & 3))) & 1);
        }
    }
    if (blockIdx.x == 0) {
        if (tid < s.head) out[tid] = feature_at<CH>(s.px, tid) > t;
        if (tid < s.HW - s.tail_at) out[s.tail_at + tid] = feature_at<CH>(s.px, s.tail_at + tid) > t;
    }
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

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool images_ok(int N, int H, int W) { return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1LL << 31); }
dim3 pixel_grid(int N, long long HW) {
    const long long want = (HW / kRun + kThreads - 1) / kThreads, cap = kMaxBlocks / N;
    const long long per = want < cap ? want : cap;
    return dim3((unsigned)(per > 1 ? per : 1), (unsigned)N);
}

}  // namespace

extern "C" int cs_tissue_histogram(const uint8_t* images_hwc, int N, int H, int W, int channel, int64_t* hist, void* stream) {
    CS_CHECK_ARG(images_ok(N, H, W), "tissue_histogram: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(channel == CS_TISSUE_CHROMA || channel == CS_TISSUE_DARKNESS, "tissue_histogram: unknown channel");
    CS_CHECK_ARG(images_hwc && hist, "tissue_histogram: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(hist) & 7) == 0, "tissue_histogram: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    if (channel == CS_TISSUE_CHROMA) hipLaunchKernelGGL(tissue_histogram_kernel<CS_TISSUE_CHROMA>, pixel_grid(N, HW), dim3(kThreads), 0, st, images_hwc, HW, h);
    else hipLaunchKernelGGL(tissue_histogram_kernel<CS_TISSUE_DARKNESS>, pixel_grid(N, HW), dim3(kThreads), 0, st, images_hwc, HW, h);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_tissue_mask(const uint8_t* images_hwc, int N, int H, int W, int channel, const int32_t* thr, uint8_t* mask, void* stream) {
    CS_CHECK_ARG(images_ok(N, H, W), "tissue_mask: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(channel == CS_TISSUE_CHROMA || channel == CS_TISSUE_DARKNESS, "tissue_mask: unknown channel");
    CS_CHECK_ARG(images_hwc && thr && mask, "tissue_mask: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(thr) & 3) == 0, "tissue_mask: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W;
    if (channel == CS_TISSUE_CHROMA) hipLaunchKernelGGL(tissue_mask_kernel<CS_TISSUE_CHROMA>, pixel_grid(N, HW), dim3(kThreads), 0, st, images_hwc, HW, thr, mask);
    else hipLaunchKernelGGL(tissue_mask_kernel<CS_TISSUE_DARKNESS>, pixel_grid(N, HW), dim3(kThreads), 0, st, images_hwc, HW, thr, mask);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_tissue_coverage(const uint8_t* mask, int N, int H, int W, const int32_t* tile_img, const int32_t* tile_rc, long long T, int ph,
                                  int pw, int32_t* cover, void* stream) {
    CS_CHECK_ARG(images_ok(N, H, W), "tissue_coverage: need 0 < N <= 65535 masks of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(T >= 0 && T < (1LL << 31) && ph > 0 && pw > 0, "tissue_coverage: need 0 <= T < 2^31 windows of ph, pw > 0");
    CS_CHECK_ARG(mask && ((tile_img && tile_rc && cover) || T == 0), "tissue_coverage: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(tile_img) & 3) == 0 && (reinterpret_cast<uintptr_t>(tile_rc) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(cover) & 3) == 0, "tissue_coverage: misaligned argument");
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
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(cover) & 3) == 0 && (reinterpret_cast<uintptr_t>(selected) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(n_selected) & 3) == 0, "tissue_select: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tissue_select_kernel, dim3(1), dim3(kThreads), 0, st, cover, T, min_pixels, selected, n_selected);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
