// Scoring of detected cell centres against annotated ones (test_seg.py:120-141 get_prf1 with metrics/metrics.py:56-66): a greedy
// assignment in the order of the detections.  Per image, every detection takes the nearest annotation that no earlier detection
// has taken (lowest index among equally near ones) and keeps it when dr^2 + dc^2 <= radius2; tp = matches, fp = detections scored
// - tp, fn = annotations left over.  Coordinates are integers, so every comparison is one of squared distances in integers: no
// float decides anything.  Only annotations with |dr| <= R and |dc| <= R, R = isqrt(radius2) <= 46340, can match; they are the only
// ones whose distance is ever squared, so d2 <= 2 R^2 < 2^32 fits an unsigned 32-bit word.
//
// One launch, one workgroup of 256 threads per image, branching uniformly on the image's n_gt:
//   wave path   n_gt <= 64: wave 0 alone, lane j holds annotation j, the flags are one 64-bit mask.  Per detection a __shfl_xor
//               min-reduction of d2 over the unflagged lanes within the radius, then the lowest lane that holds the minimum (a
//               ballot): the minimum of the key (d2, j).  No LDS, no barrier.
//   block path  any n_gt: thread t scans annotations t, t + 256, ... (|d| > R rejected before anything is squared), the packed
//               key d2 << 32 | j is min-reduced in the wave by __shfl_xor and across the four waves through LDS.  Up to 4096
//               annotations live in LDS with their flag bits; beyond that the coordinates are read from global memory and the flag
//               bits live in the workspace (zeroed by the workgroup itself).  The thread that scans annotation j is the one that
//               sets its flag and writes `match`, and the only one that ever tests that bit again, so one barrier per detection
//               (the key slots are double-buffered) is all the loop needs.  fn = popcount of the clear flags.
// Images share nothing and every reduction is a minimum of distinct integers: the result does not depend on scheduling.
#include <limits.h>
#include "cs_common.h"
#include "cs_points.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsGt = 4096;                       // annotations of one image held in LDS
constexpr uint32_t kFar = 0xffffffffu;             // no candidate: valid d2 are <= radius2 < 2^31
constexpr unsigned long long kNoKey = ~0ull;

struct Det {
    int r, c;
    bool ok;                                       // both coordinates fit int32
};
__device__ __forceinline__ Det load_det(const int64_t* __restrict__ hat, long long i) {
    const long long r = hat[2 * i], c = hat[2 * i + 1];
    return {(int)r, (int)c, r == (long long)(int)r && c == (long long)(int)c};
}

// d2 of annotation (gr, gc) from the detection where it lies within the radius, kFar elsewhere
__device__ __forceinline__ uint32_t near_d2(int gr, int gc, const Det& d, int R, uint32_t radius2) {
    const long long dr = (long long)gr - d.r, dc = (long long)gc - d.c;
    if (dr > R || dr < -R || dc > R || dc < -R) return kFar;
    const uint32_t d2 = (uint32_t)(dr * dr + dc * dc);
    return d2 <= radius2 ? d2 : kFar;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct Image {
    const int64_t* hat;                            // the image's detections
    const int32_t* gt;                             // the image's annotations
    int32_t* match;                                // the image's slice of `match` (or NULL)
    int n_eff, n_gt;                               // detections scored, annotations
};

// wave 0 only; returns tp (uniform) and leaves the flags in `flagged`
__device__ __forceinline__ int wave_path(const Image& im, int R, uint32_t radius2, unsigned long long* flagged_out) {
    const int lane = threadIdx.x;
    const bool have = lane < im.n_gt;
    int gr = 0, gc = 0;
    if (have) {
        const int2 p = *reinterpret_cast<const int2*>(im.gt + 2 * lane);
        gr = p.x;
        gc = p.y;
    }
    unsigned long long flagged = 0;
    int tp = 0;
    for (int i = 0; i < im.n_eff; ++i) {
        const Det d = load_det(im.hat, i);
        uint32_t d2 = kFar;
        if (have && d.ok && !((flagged >> lane) & 1ull)) d2 = near_d2(gr, gc, d, R, radius2);
        const uint32_t best = wave_min_u32(d2);
        const unsigned long long holders = __ballot(d2 == best && best != kFar);
        int j = -1;
        if (holders) {
            j = __ffsll((long long)holders) - 1;
            flagged |= 1ull << j;
            ++tp;
        }
        if (lane == 0 && im.match) im.match[i] = j;
    }
    *flagged_out = flagged;
    return tp;
}

// every thread of the workgroup; IN_LDS: the annotations and their flags are in LDS, else in global memory (flags: workspace words)
template <bool IN_LDS>
__device__ __forceinline__ void block_path(const Image& im, int R, uint32_t radius2, int* s_r, int* s_c, uint32_t* s_flag,
                                           unsigned long long (*s_key)[kWaves], int* s_sum, uint32_t* g_flag, int32_t* counts) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int words = (im.n_gt + 31) >> 5;
    if (IN_LDS) {
        for (int e = tid; e < 2 * im.n_gt; e += kThreads) ((e & 1) ? s_c : s_r)[e >> 1] = im.gt[e];
        for (int w = tid; w < words; w += kThreads) s_flag[w] = 0;
    } else {
        for (int w = tid; w < words; w += kThreads) __hip_atomic_store(g_flag + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
    }
    __syncthreads();
    int tp = 0;
    for (int i = 0; i < im.n_eff; ++i) {
        const Det d = load_det(im.hat, i);
        unsigned long long key = kNoKey;
        if (d.ok) {
            for (int j = tid; j < im.n_gt; j += kThreads) {
                int gr, gc;
                if (IN_LDS) {
                    gr = s_r[j];
                    gc = s_c[j];
                } else {
                    const int2 p = *reinterpret_cast<const int2*>(im.gt + 2 * (long long)j);
                    gr = p.x;
                    gc = p.y;
                }
                const uint32_t d2 = near_d2(gr, gc, d, R, radius2);
                if (d2 == kFar) continue;
                // bit j was set, if ever, by this very thread: no other thread's write is waited for
                const uint32_t f = IN_LDS ? s_flag[j >> 5] : __hip_atomic_load(g_flag + (j >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((f >> (j & 31)) & 1u) continue;
                const unsigned long long k = ((unsigned long long)d2 << 32) | (uint32_t)j;
                key = k < key ? k : key;
            }
        }
        key = wave_min_u64(key);
        unsigned long long* slot = s_key[i & 1];   // the other buffer may still be read by a wave that is one detection behind
        if (lane == 0) slot[wave] = key;
        __syncthreads();
        unsigned long long best = slot[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = slot[w] < best ? slot[w] : best;
        if (best != kNoKey) {
            const int j = (int)(uint32_t)best;
            if ((j & (kThreads - 1)) == tid) {
                if (IN_LDS) atomicOr(s_flag + (j >> 5), 1u << (j & 31));
                else __hip_atomic_fetch_or(g_flag + (j >> 5), 1u << (j & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (im.match) im.match[i] = j;
            }
            ++tp;
        } else if (tid == 0 && im.match) {
            im.match[i] = -1;
        }
    }
    if (!IN_LDS) __threadfence();
    __syncthreads();
    int clear = 0;
    for (int w = tid; w < words; w += kThreads) {
        const uint32_t f = IN_LDS ? s_flag[w] : __hip_atomic_load(g_flag + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t valid = (w == words - 1 && (im.n_gt & 31)) ? (1u << (im.n_gt & 31)) - 1u : ~0u;
        clear += __popc(~f & valid);
    }
    clear = wave_sum_i32(clear);
    if (lane == 0) s_sum[wave] = clear;
    __syncthreads();
    if (tid == 0) {
        int fn = 0;
        for (int w = 0; w < kWaves; ++w) fn += s_sum[w];
        counts[0] = tp;
        counts[1] = im.n_eff - tp;
        counts[2] = fn;
    }
}

// grid (N), kThreads threads.  The detections scored are a window of the ragged point set of cs_points.h, the annotations a window
// without limits.  An image with a window that is not ok, or whose flag words would not fit the workspace, reports counts
// (-1, -1, -1) and touches nothing else.
__global__ __launch_bounds__(kThreads) void score_kernel(const int64_t* __restrict__ hat, const int64_t* __restrict__ hat_off,
                                                         const int32_t* __restrict__ hat_limit, const int32_t* __restrict__ gt,
                                                         const int64_t* __restrict__ gt_off, int R, uint32_t radius2, int force_block,
                                                         int32_t* __restrict__ counts_all, int32_t* __restrict__ match,
                                                         uint32_t* __restrict__ ws, long long ws_words) {
    __shared__ int s_r[kLdsGt];
    __shared__ int s_c[kLdsGt];
    __shared__ uint32_t s_flag[kLdsGt / 32];
    __shared__ unsigned long long s_key[2][kWaves];
    __shared__ int s_sum[kWaves];
    const int n = blockIdx.x, tid = threadIdx.x;
    int32_t* counts = counts_all + 3 * (long long)n;
    // the entry point knows the rows of neither buffer: any window of 0 <= n < 2^31 rows from a row >= 0 on is taken
    const PointWindow hw = point_window(hat_off[n], hat_off[n + 1], LLONG_MAX, hat_limit, n);
    const PointWindow gw = point_window(gt_off[n], gt_off[n + 1], LLONG_MAX, nullptr, n);
    const long long flag0 = (gw.o0 >> 5) + n;                             // first flag word of the image in the workspace
    if (!hw.ok || !gw.ok || (gw.count > kLdsGt && flag0 + (((long long)gw.count + 31) >> 5) > ws_words)) {
        if (tid < 3) counts[tid] = -1;
        return;
    }
    const int n_hat = hw.count, n_eff = hw.kept;
    Image im;
    im.hat = hat + 2 * hw.o0;
    im.gt = gt + 2 * gw.o0;
    im.match = match ? match + hw.o0 : nullptr;
    im.n_eff = n_eff;
    im.n_gt = gw.count;
    if (match)
        for (int i = n_eff + tid; i < n_hat; i += kThreads) im.match[i] = -2;
    if (im.n_gt <= 64 && !force_block) {
        if (tid >= 64) return;
        unsigned long long flagged;
        const int tp = wave_path(im, R, radius2, &flagged);
        if (tid == 0) {
            counts[0] = tp;
            counts[1] = n_eff - tp;
            counts[2] = im.n_gt - __popcll(flagged);
        }
        return;
    }
    if (im.n_gt <= kLdsGt) block_path<true>(im, R, radius2, s_r, s_c, s_flag, s_key, s_sum, nullptr, counts);
    else block_path<false>(im, R, radius2, s_r, s_c, s_flag, s_key, s_sum, ws + flag0, counts);
}

}  // namespace

// workspace: the flag bits of the images with more than 4096 annotations, image n from word gt_off[n] / 32 + n on
extern "C" size_t cs_score_workspace(int N, long long total_gt) {
    if (N <= 0 || N > 65535 || total_gt < 0) return 0;
    return cs_align16(((size_t)(total_gt >> 5) + (size_t)N + 1) * 4);
}

extern "C" int cs_score_points(const int64_t* hat, const int64_t* hat_off, const int32_t* hat_limit, const int32_t* gt,
                               const int64_t* gt_off, int N, int radius2, int flags, int32_t* counts, int32_t* match, void* workspace,
                               size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(N > 0 && N <= 65535, "score_points: need 0 < N <= 65535");
    CS_CHECK_ARG(hat_off && gt_off && counts && workspace, "score_points: NULL argument");
    CS_CHECK_ARG(radius2 >= 0, "score_points: radius2 must be non-negative and below 2^31");
    CS_CHECK_ARG((flags & ~1) == 0, "score_points: unknown flag bits");
    CS_CHECK_ARG(workspace_bytes >= cs_score_workspace(N, 0), "score_points: workspace too small");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(gt) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(hat) & 7) == 0, "score_points: misaligned argument");
    int R = 0;                                                            // isqrt(radius2)
    while ((long long)(R + 1) * (R + 1) <= radius2) ++R;
    hipLaunchKernelGGL(score_kernel, dim3(N), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), hat, hat_off, hat_limit, gt, gt_off,
                       R, (uint32_t)radius2, flags & 1, counts, match, reinterpret_cast<uint32_t*>(workspace),
                       (long long)(workspace_bytes / 4));
    CS_LAUNCH_CHECK();
    return CS_OK;
}
