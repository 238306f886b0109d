// The pixel-run walker of the per-pixel passes over uint8 RGB images [N][H][W][3] (tissue.hip, stain.hip, render.hip).
//
// A thread takes kPixelRun = 16 consecutive pixels = 48 bytes per step, as three 16-byte loads.  Nothing is asked of the alignment
// of the images: 3 is invertible mod 16 (3 * 11 = 33 = 1), so among the first 16 pixels of any span there is one whose first byte
// lies on a 16-byte boundary -- pixel k with px + 3 k = 0 (mod 16), k = 11 * (-px) (mod 16) -- and from it on every run of 16
// pixels is three aligned 16-byte words.  The fewer than 16 pixels before it (the head) and the fewer than 16 after the last whole
// run (the tail) are taken one by one, a pixel per thread, by the first workgroup of the span (blockIdx.x == 0).  What goes with
// the pixels -- a mask or a map read beside them, the output -- starts wherever its tensor happens to start: it moves as 16-byte
// words, as dwords or as bytes, by the address its first run meets (access_width), which is uniform over the span because every
// run lies a multiple of 16 bytes after the first.  Grids are capped (kMaxBlocks) and stride over the runs.
//
// The second half is the workgroup's histogram in LDS for passes that count pixels by a value: `copies` sub-histograms (a power of
// two; lane & (copies - 1) picks one, so neighbouring lanes do not meet on a word) of `stride` = bins + 1 words each, so that one
// bin of the copies falls into different banks; the workgroup folds the copies and adds the non-zero sums to memory with one 64-bit
// integer atomic each.
#pragma once
#include "cs_common.h"

constexpr int kPixelRun = 16;                      // pixels per thread and step
constexpr int kMaxBlocks = 2048;                   // of one pixel pass, all images together (an image has at least one)

// `count` pixels from px on as [0, head) single pixels, `runs` runs of kPixelRun pixels from the 16-byte boundary at pixel `head`
// on, [tail_at, count) single pixels
struct PixelSpan {
    const uint8_t* px;
    long long head, runs, tail_at, count;
};
__device__ __forceinline__ PixelSpan pixel_span(const uint8_t* __restrict__ px, long long count) {
    PixelSpan s;
    s.px = px;
    s.count = count;
    const long long k = (11 * ((16 - (int)(reinterpret_cast<uintptr_t>(px) & 15)) & 15)) & 15;
    s.head = k < count ? k : count;
    s.runs = (count - s.head) / kPixelRun;
    s.tail_at = s.head + s.runs * kPixelRun;
    return s;
}

// the widest access every run of a span allows when its first run starts at p: 16, 4 or 1 bytes
__device__ __forceinline__ int access_width(const void* p) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(p);
    return (at & 15) == 0 ? 16 : (at & 3) == 0 ? 4 : 1;
}
// byte o of a run of words
template <int NW>
__device__ __forceinline__ int byte_of(const uint32_t (&w)[NW], int o) { return (w[o >> 2] >> (8 * (o & 3))) & 255; }

// the 16 pixels in the 48 bytes at p (16-byte aligned)
__device__ __forceinline__ void load_pixels(const uint8_t* __restrict__ p, uint32_t (&w)[12]) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1], c = reinterpret_cast<const uint4*>(p)[2];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w, w[8] = c.x, w[9] = c.y, w[10] = c.z, w[11] = c.w;
}
// the 16 bytes at q, one per pixel of a run
__device__ __forceinline__ void load_bytes16(const uint8_t* __restrict__ q, int width, uint32_t (&w)[4]) {
    if (width == 16) {
        const uint4 a = *reinterpret_cast<const uint4*>(q);
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    } else if (width == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = reinterpret_cast<const uint32_t*>(q)[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = q[4 * j] | (uint32_t)q[4 * j + 1] << 8 | (uint32_t)q[4 * j + 2] << 16 | (uint32_t)q[4 * j + 3] << 24;
    }
}
// NW words (a multiple of 4) to q
template <int NW>
__device__ __forceinline__ void store_words(uint8_t* __restrict__ q, int width, const uint32_t (&w)[NW]) {
    if (width == 16) {
#pragma unroll
        for (int j = 0; j < NW / 4; ++j) reinterpret_cast<uint4*>(q)[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
    } else if (width == 4) {
#pragma unroll
        for (int j = 0; j < NW; ++j) reinterpret_cast<uint32_t*>(q)[j] = w[j];
    } else {
#pragma unroll
        for (int i = 0; i < 4 * NW; ++i) q[i] = (uint8_t)byte_of(w, i);
    }
}

// Walks the span with workgroups of THREADS, the grid's x striding over the runs: run(g, w) for the runs of this thread, with the
// 12 words of run g loaded (its to overwrite); single(i) for the pixels before the first and after the last run, which the first workgroup takes, a
// pixel per thread.
template <int THREADS, typename Run, typename Single>
__device__ __forceinline__ void for_pixels(const PixelSpan& s, Run run, Single single) {
    for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < s.runs; g += (long long)gridDim.x * THREADS) {
        uint32_t w[12];
        load_pixels(s.px + 3 * (s.head + kPixelRun * g), w);
        run(g, w);
    }
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x;
        if (t < s.head) single(t);
        if (t < s.count - s.tail_at) single(s.tail_at + t);
    }
}

// ---- the workgroup's sub-histograms: s_hist holds copies * stride words, stride = bins + 1 ------------------------------------------
// zeroes them; a barrier of the caller's follows before the first count
template <int THREADS>
__device__ __forceinline__ void hist_zero(uint32_t* s_hist, int copies, int stride) {
    for (int i = threadIdx.x; i < copies * stride; i += THREADS) s_hist[i] = 0;
}
// the copy this thread counts into, with LDS atomics
__device__ __forceinline__ uint32_t* hist_mine(uint32_t* s_hist, int copies, int stride) { return s_hist + (threadIdx.x & (copies - 1)) * stride; }
// after the last count: folds the copies and adds the non-zero sums to hist[0 .. stride - 1).  A workgroup's pixels are fewer than 2^31.
template <int THREADS>
__device__ __forceinline__ void hist_flush(const uint32_t* s_hist, int copies, int stride, unsigned long long* __restrict__ hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < stride - 1; b += THREADS) {
        uint32_t sum = 0;
        for (int c = 0; c < copies; ++c) sum += s_hist[c * stride + b];
        if (sum) atomicAdd(hist + b, (unsigned long long)sum);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
static inline bool pixel_images_ok(int N, int H, int W) { return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1LL << 31); }
// the same for a pass that walks the whole batch as one span
static inline bool pixel_batch_ok(int N, int H, int W) { return pixel_images_ok(N, H, W) && (long long)N * H * W < (1LL << 31); }
// grid (blocks per image, N) over N spans of HW pixels each; a batch walked as one span is N = 1
static inline dim3 pixel_grid(int N, long long HW, int threads) {
    const long long want = (HW / kPixelRun + threads - 1) / threads, cap = kMaxBlocks / N;
    const long long per = want < cap ? want : cap;
    return dim3((unsigned)(per > 1 ? per : 1), (unsigned)N);
}
