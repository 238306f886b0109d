// Stain separation and Macenko stain normalisation (stain.py is the public API): per-pixel passes over uint8 RGB slides plus the
// integer moments and the two histograms the estimate of a slide's stain vectors needs.  Five launches:
//   moments    int64 [10] per image: the number of kept pixels and the first and second moments of their quantised optical density
//              (r, g, b, rr, rg, rb, gg, gb, bb).  Integer only: 8 pixels' products fit 32 bits (8 * 22713^2 < 2^32), a step's 16
//              linear terms as well, and both go to 64-bit registers from there; a wave folds by shuffles, the workgroup through
//              LDS, and ten 64-bit integer atomics per workgroup reach memory.  The bits do not depend on the launch geometry.
//   angle_hist int64 [B] per image: kept pixels by the angle of their projection on a plane, phi = atan2f(od.V1, od.V0).
//   conc_hist  int64 [2][Bc] per image: kept pixels by each of two concentrations c = P od.
//              Both count into the sub-histograms of cs_pixels.h, as many copies as kMaxBins words of LDS hold.
//   apply      uint8 RGB out = clamp(rint(Io exp(-(A od))), 0, 255) for every pixel, as exp2(log2 Io - (A od) log2 e) with log2 Io
//              from the host and log2 e folded into A: one v_exp_f32 per channel.  Its error stays below 10^-3 levels.
//   separate   c = P od for every pixel, K = 2 or 3 stains, as fp32 or as uint8 clamp(rint(255 c / conc_max), 0, 255).
// The optical density is a table of 256 integers made once on the host, od_q[v] = rint(4096 ln(Io / (v + 1))), kept in LDS; the
// float od is od_q / 4096, exact in fp32, and no kernel calls log.  A pixel is KEPT when none of its three od_q is below beta_q
// and, with a mask, its mask byte is non-zero.
// The pixels are walked by cs_pixels.h (runs of 16 pixels as three 16-byte loads, single pixels on either side), which also keeps the
// sub-histograms of the two histogram kernels; nothing is asked of the alignment of the images, the mask or the outputs.
#include <cmath>

#include "cs_common.h"
#include "cs_pixels.h"

namespace {

constexpr int kThreads = 256;                      // also the entries of the od table: thread v loads entry v
constexpr int kMaxBins = 8192;                     // histogram words of one copy in LDS: B, or 2 Bc
constexpr int kMaxCopies = 16;
constexpr int kMoments = 10;
constexpr float kOdUnit = 1.0f / 4096.0f;
constexpr float kHalfPi = 1.57079632679489661923f;
constexpr float kLog2e = 1.44269504088896340736f;

// a row of a 3-column matrix times the float optical density of a pixel, in this order everywhere
__device__ __forceinline__ float dot3(const float* __restrict__ a, float r, float g, float b) { return fmaf(b, a[2], fmaf(g, a[1], r * a[0])); }
// a float as a uint8 level: NaN becomes 0
__device__ __forceinline__ uint32_t level(float v) { return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }
// floor(x) as a bin of `bins`, clamped: NaN becomes bin 0
__device__ __forceinline__ int bin_of(float x, int bins) { return (int)fminf(fmaxf(floorf(x), 0.0f), (float)(bins - 1)); }

// The kept pixels of the image: keep(qr, qg, qb) for each, with its three quantised optical densities.  `flush(i)` follows pixel
// i of a run (and every single pixel, as i = kPixelRun - 1), kept or not.
template <typename Keep, typename Flush>
__device__ __forceinline__ void for_kept_pixels(const PixelSpan& s, const int32_t* __restrict__ od, int beta_q, const uint8_t* __restrict__ mask,
                                                Keep keep, Flush flush) {
    const int width = mask ? access_width(mask + s.head) : 0;
    auto take = [&](int r, int g, int b, bool on) {
        const int qr = od[r], qg = od[g], qb = od[b];
        if (on && min(qr, min(qg, qb)) >= beta_q) keep(qr, qg, qb);
    };
    for_pixels<kThreads>(
        s,
        [&](long long g, const uint32_t(&w)[12]) {
            uint32_t m[4] = {~0u, ~0u, ~0u, ~0u};
            if (mask) load_bytes16(mask + s.head + kPixelRun * g, width, m);
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) {
                take(byte_of(w, 3 * i), byte_of(w, 3 * i + 1), byte_of(w, 3 * i + 2), byte_of(m, i) != 0);
                flush(i);
            }
        },
        [&](long long i) {
            take(s.px[3 * i], s.px[3 * i + 1], s.px[3 * i + 2], !mask || mask[i] != 0);
            flush(kPixelRun - 1);
        });
}

// grid (blocks per image, N)
__global__ __launch_bounds__(kThreads) void stain_moments_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ od_q,
                                                                 int beta_q, const uint8_t* __restrict__ mask,
                                                                 unsigned long long* __restrict__ moments) {
    __shared__ int32_t s_od[256];
    __shared__ unsigned long long s_part[kThreads / 64][kMoments];
    const int n = blockIdx.y, tid = threadIdx.x;
    s_od[tid] = od_q[tid];
    __syncthreads();
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    unsigned long long acc[kMoments] = {};
    uint32_t lin[4] = {}, quad[6] = {};             // of the pixels since the last flush: at most 16 and 8 of them
    for_kept_pixels(
        s, s_od, beta_q, mask ? mask + (long long)n * HW : nullptr,
        [&](int qr, int qg, int qb) {
            lin[0] += 1, lin[1] += qr, lin[2] += qg, lin[3] += qb;
            quad[0] += __umul24(qr, qr), quad[1] += __umul24(qr, qg), quad[2] += __umul24(qr, qb);
            quad[3] += __umul24(qg, qg), quad[4] += __umul24(qg, qb), quad[5] += __umul24(qb, qb);
        },
        [&](int i) {
            if ((i & 7) == 7) {
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[4 + k] += quad[k], quad[k] = 0;
            }
            if (i == kPixelRun - 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += lin[k], lin[k] = 0;
            }
        });
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
        long long v = (long long)acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) s_part[tid >> 6][k] = (unsigned long long)v;
    }
    __syncthreads();
    if (tid < kMoments) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) sum += s_part[w][tid];
        if (sum) atomicAdd(moments + (long long)n * kMoments + tid, sum);
    }
}

// grid (blocks per image, N), dynamic LDS copies * (TB + 1) words with TB = bins (angle) or 2 bins (concentrations).  `M` holds six
// floats per image: V [3][2] for the angle (od V), P [2][3] for the concentrations (P od).
template <bool CONC>
__global__ __launch_bounds__(kThreads) void stain_hist_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ od_q,
                                                              int beta_q, const uint8_t* __restrict__ mask, const float* __restrict__ M, int bins,
                                                              int copies, float scale, unsigned long long* __restrict__ hist) {
    __shared__ int32_t s_od[256];
    extern __shared__ uint32_t s_hist[];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int TB = CONC ? 2 * bins : bins, stride = TB + 1;
    s_od[tid] = od_q[tid];
    hist_zero<kThreads>(s_hist, copies, stride);
    __syncthreads();
    uint32_t* mine = hist_mine(s_hist, copies, stride);
    float a0[3], a1[3];                            // the two rows that meet the od of a pixel
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a0[j] = M[6 * n + (CONC ? j : 2 * j)];
        a1[j] = M[6 * n + (CONC ? 3 + j : 2 * j + 1)];
    }
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    for_kept_pixels(
        s, s_od, beta_q, mask ? mask + (long long)n * HW : nullptr,
        [&](int qr, int qg, int qb) {
            const float r = qr * kOdUnit, g = qg * kOdUnit, b = qb * kOdUnit;
            const float c0 = dot3(a0, r, g, b), c1 = dot3(a1, r, g, b);
            if (CONC) {
                atomicAdd(mine + bin_of(c0 * scale, bins), 1u);
                atomicAdd(mine + bins + bin_of(c1 * scale, bins), 1u);
            } else {
                atomicAdd(mine + bin_of((atan2f(c1, c0) + kHalfPi) * scale, bins), 1u);
            }
        },
        [](int) {});
    hist_flush<kThreads>(s_hist, copies, stride, hist + (long long)n * TB);
}

// grid (blocks per image, N)
__global__ __launch_bounds__(kThreads) void stain_apply_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ od_q,
                                                               const float* __restrict__ A, float lg_Io, uint8_t* __restrict__ out) {
    __shared__ float s_od[256];
    const int n = blockIdx.y, tid = threadIdx.x;
    s_od[tid] = od_q[tid] * kOdUnit;
    __syncthreads();
    float a[9];                                    // Io exp(-x) = exp2(log2 Io - x log2 e): one v_exp_f32 per channel, no multiply by Io
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = -kLog2e * A[9 * n + j];
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    uint8_t* o = out + (long long)n * HW * 3;
    const int width = access_width(o + 3 * s.head);
    auto pixel = [&](int r8, int g8, int b8, int c) {
        const float* row = a + 3 * c;
        return level(__builtin_amdgcn_exp2f(fmaf(s_od[b8], row[2], fmaf(s_od[g8], row[1], fmaf(s_od[r8], row[0], lg_Io)))));
    };
    for_pixels<kThreads>(
        s,
        [&](long long g, const uint32_t(&w)[12]) {
            uint32_t v[12] = {};
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) {
                const int r8 = byte_of(w, 3 * i), g8 = byte_of(w, 3 * i + 1), b8 = byte_of(w, 3 * i + 2);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[(3 * i + c) >> 2] |= pixel(r8, g8, b8, c) << (8 * ((3 * i + c) & 3));
            }
            store_words(o + 3 * (s.head + kPixelRun * g), width, v);
        },
        [&](long long i) {
            const int r8 = s.px[3 * i], g8 = s.px[3 * i + 1], b8 = s.px[3 * i + 2];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * i + c] = (uint8_t)pixel(r8, g8, b8, c);
        });
}

// grid (blocks per image, N); out is uint8 (U8, `scale` = 255 / conc_max) or fp32 [N][H][W][K]
template <int K, bool U8>
__global__ __launch_bounds__(kThreads) void stain_separate_kernel(const uint8_t* __restrict__ images, long long HW, const int32_t* __restrict__ od_q,
                                                                  const float* __restrict__ P, float scale, void* __restrict__ out) {
    __shared__ float s_od[256];
    const int n = blockIdx.y, tid = threadIdx.x;
    s_od[tid] = od_q[tid] * kOdUnit;
    __syncthreads();
    float p[3 * K];
#pragma unroll
    for (int j = 0; j < 3 * K; ++j) p[j] = P[3 * K * n + j];
    const PixelSpan s = pixel_span(images + (long long)n * HW * 3, HW);
    constexpr int kItem = U8 ? 1 : 4;              // bytes per value
    uint8_t* o = static_cast<uint8_t*>(out) + (long long)n * HW * K * kItem;
    const int width = access_width(o + (long long)K * kItem * s.head);
    auto conc = [&](int r8, int g8, int b8, int k) {
        return dot3(p + 3 * k, s_od[r8], s_od[g8], s_od[b8]);
    };
    for_pixels<kThreads>(
        s,
        [&](long long g, const uint32_t(&w)[12]) {
            uint32_t v[kPixelRun * K * kItem / 4] = {};
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) {
                const int r8 = byte_of(w, 3 * i), g8 = byte_of(w, 3 * i + 1), b8 = byte_of(w, 3 * i + 2);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float c = conc(r8, g8, b8, k);
                    if (U8) v[(K * i + k) >> 2] |= level(c * scale) << (8 * ((K * i + k) & 3));
                    else v[K * i + k] = __float_as_uint(c);
                }
            }
            store_words(o + (long long)K * kItem * (s.head + kPixelRun * g), width, v);
        },
        [&](long long i) {
            const int r8 = s.px[3 * i], g8 = s.px[3 * i + 1], b8 = s.px[3 * i + 2];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float c = conc(r8, g8, b8, k);
                if (U8) o[K * i + k] = (uint8_t)level(c * scale);
                else reinterpret_cast<float*>(o)[K * i + k] = c;
            }
        });
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the sub-histograms of a workgroup with TB bins each: a power of two, as many as kMaxBins words hold
int hist_copies(int TB) {
    int c = 1;
    while (2 * c <= kMaxCopies && 2 * c * TB <= kMaxBins) c *= 2;
    return c;
}

template <bool CONC>
int launch_hist(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask, const float* M, int bins,
                float scale, int64_t* hist, void* stream) {
    const int TB = CONC ? 2 * bins : bins, copies = hist_copies(TB);
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(stain_hist_kernel<CONC>, pixel_grid(N, HW, kThreads), dim3(kThreads), (size_t)copies * (TB + 1) * sizeof(uint32_t),
                       reinterpret_cast<hipStream_t>(stream), images_hwc, HW, od_q, beta_q, mask, M, bins, copies, scale,
                       reinterpret_cast<unsigned long long*>(hist));
    CS_LAUNCH_CHECK();
    return CS_OK;
}

}  // namespace

extern "C" int cs_stain_moments(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask,
                                int64_t* moments, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "stain_moments: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(images_hwc && od_q && moments, "stain_moments: NULL argument");
    CS_CHECK_ARG(aligned(od_q, 4) && aligned(moments, 8), "stain_moments: misaligned argument");
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(stain_moments_kernel, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), images_hwc, HW, od_q,
                       beta_q, mask, reinterpret_cast<unsigned long long*>(moments));
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stain_angle_hist(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask,
                                   const float* V, int bins, int64_t* hist, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "stain_angle_hist: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(bins > 0 && bins <= kMaxBins, "stain_angle_hist: need 0 < bins <= 8192");
    CS_CHECK_ARG(images_hwc && od_q && V && hist, "stain_angle_hist: NULL argument");
    CS_CHECK_ARG(aligned(od_q, 4) && aligned(V, 4) && aligned(hist, 8), "stain_angle_hist: misaligned argument");
    return launch_hist<false>(images_hwc, N, H, W, od_q, beta_q, mask, V, bins, (float)(bins / 3.14159265358979323846), hist, stream);
}

extern "C" int cs_stain_conc_hist(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask,
                                  const float* P, int bins, float conc_max, int64_t* hist, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "stain_conc_hist: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(bins > 0 && 2 * bins <= kMaxBins, "stain_conc_hist: need 0 < bins <= 4096");
    CS_CHECK_ARG(conc_max > 0 && conc_max <= 3.0e38f, "stain_conc_hist: conc_max must be positive and finite");
    CS_CHECK_ARG(images_hwc && od_q && P && hist, "stain_conc_hist: NULL argument");
    CS_CHECK_ARG(aligned(od_q, 4) && aligned(P, 4) && aligned(hist, 8), "stain_conc_hist: misaligned argument");
    return launch_hist<true>(images_hwc, N, H, W, od_q, beta_q, mask, P, bins, (float)((double)bins / conc_max), hist, stream);
}

extern "C" int cs_stain_apply(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, const float* A, float Io, uint8_t* out,
                              void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "stain_apply: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(Io > 0 && Io <= 256.0f, "stain_apply: need 0 < Io <= 256");
    CS_CHECK_ARG(images_hwc && od_q && A && out, "stain_apply: NULL argument");
    CS_CHECK_ARG(aligned(od_q, 4) && aligned(A, 4), "stain_apply: misaligned argument");
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(stain_apply_kernel, pixel_grid(N, HW, kThreads), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), images_hwc, HW, od_q, A,
                       (float)std::log2((double)Io), out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stain_separate(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, const float* P, int K, int as_u8,
                                 float conc_max, void* out, void* stream) {
    CS_CHECK_ARG(pixel_images_ok(N, H, W), "stain_separate: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(K == 2 || K == 3, "stain_separate: need K = 2 or 3 stains");
    CS_CHECK_ARG(as_u8 == 0 || as_u8 == 1, "stain_separate: as_u8 is 0 (fp32 out) or 1 (uint8 out)");
    CS_CHECK_ARG(!as_u8 || (conc_max > 0 && conc_max <= 3.0e38f), "stain_separate: conc_max must be positive and finite");
    CS_CHECK_ARG(images_hwc && od_q && P && out, "stain_separate: NULL argument");
    CS_CHECK_ARG(aligned(od_q, 4) && aligned(P, 4) && (as_u8 || aligned(out, 4)), "stain_separate: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W;
    const dim3 grid = pixel_grid(N, HW, kThreads);
    const float scale = as_u8 ? (float)(255.0 / conc_max) : 0.0f;
    if (K == 2 && as_u8) hipLaunchKernelGGL((stain_separate_kernel<2, true>), grid, dim3(kThreads), 0, st, images_hwc, HW, od_q, P, scale, out);
    else if (K == 2) hipLaunchKernelGGL((stain_separate_kernel<2, false>), grid, dim3(kThreads), 0, st, images_hwc, HW, od_q, P, scale, out);
    else if (as_u8) hipLaunchKernelGGL((stain_separate_kernel<3, true>), grid, dim3(kThreads), 0, st, images_hwc, HW, od_q, P, scale, out);
    else hipLaunchKernelGGL((stain_separate_kernel<3, false>), grid, dim3(kThreads), 0, st, images_hwc, HW, od_q, P, scale, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
