// Augmented input staging: cs_tile_gather (resize.hip) with the two augmentations the reference trains with.
//   flips          LystoDataset(augment=True), transformIDX 1 / 2 / 3 = horizontal / vertical / both, applied to the cropped tile
//                  between ToTensor and Normalize (dataset/dataset.py:70-97, 118-120, 209-211)
//   colour jitter  Maskset(augment=True): ColorJitter between ToTensor and Normalize (dataset/dataset.py:483-495), the float-image
//                  arithmetic of torchvision 0.11.2 functional_tensor
// Per tile: crop -> /255 (fp32) -> the record's colour ops in their order, on the un-flipped crop -> flip -> (v - mean) / std.
// Everything is per pixel except the contrast op, which blends with the mean grey of the WHOLE tile as the ops in front of it left
// it.  That mean needs a pass of its own:
//   stage_mean_kernel   up to 256 workgroups per tile, 512 pixels or more each: every thread applies the ops in front of the
//                       contrast op to its pixels and adds their grey values in fp64 in a fixed order, the workgroup folds them by a
//                       fixed tree (wave butterfly, then four waves through LDS), and ONE exact-limb add per workgroup (ex_add,
//                       cs_common.h) puts the partial into the tile's accumulator: the total does not depend on the order in which
//                       the workgroups arrive.  Launched only when the caller says a record holds a contrast op; a tile without
//                       one costs its workgroups one 4-byte load.
//   stage_apply_kernel  one thread per OUTPUT pixel (3 bytes in, 16 / 32 bytes out, as tile_gather_kernel): it reads the source pixel
//                       of its flipped position, so the stores stay contiguous.  mean = fp32(sum_fp64 / n).
// The colour arithmetic is compiled with floating-point contraction off, so every operation is the rounded fp32 operation a numpy
// restatement performs (tests/augment_ref.py).  fp32 and bf16 outputs come from one templated body: bf16 = RNE(fp32 result).
// Without a jitter record and with flip code 0 the arithmetic is tile_gather_kernel's, bit for bit.
#include <limits.h>
#include "cs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMeanPixels = 512;                   // pixels of a tile per reduction workgroup, at least
constexpr int kMeanMaxBlocks = 256;                // reduction workgroups per tile (ex_add is exact up to 2^12 contributors)
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

struct Rgb { float r, g, b; };

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ToTensor: u8 / 255 in fp32
__device__ __forceinline__ Rgb load_unit(const uint8_t* px) {
    return Rgb{(float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f};
}

__device__ __forceinline__ float gray_of(const Rgb& p) {
#pragma clang fp contract(off)
    return (0.2989f * p.r + 0.587f * p.g) + 0.114f * p.b;
}

// clamp(f a + (1 - f) b, 0, 1) with g = 1 - f
__device__ __forceinline__ float blend(float a, float b, float f, float g) {
#pragma clang fp contract(off)
    return clamp01(f * a + g * b);
}

// rgb -> hsv, h <- h + f - floor(h + f), hsv -> rgb
__device__ __forceinline__ void hue_shift(Rgb& p, float f) {
#pragma clang fp contract(off)
    const float r = p.r, g = p.g, b = p.b;
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.f : maxc);
    const float d = eq ? 1.f : cr;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    float h = maxc == r ? bc - gc : (maxc == g ? (2.f + rc) - bc : (4.f + gc) - rc);
    h = h / 6.f + 1.f;                             // in (0.8, 1.9)
    h = h - truncf(h);                             // fmod(h, 1) of a positive number, exact
    const float hf = h + f;
    h = hf - floorf(hf);
    const float h6 = h * 6.f;
    const float fl = floorf(h6);                   // 0..6 (6 where h rounded up to 1)
    const float fr = h6 - fl;
    const int i = (int)fl % 6;
    const float v = maxc;
    const float pp = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * fr));
    const float t = clamp01(v * (1.f - s * (1.f - fr)));
    p.r = i == 0 ? v : i == 1 ? q : i == 2 ? pp : i == 3 ? pp : i == 4 ? t : v;
    p.g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? pp : pp;
    p.b = i == 0 ? pp : i == 1 ? pp : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// one slot of a jitter record; a code outside 0..3 is an unused slot
__device__ __forceinline__ void apply_op(int code, float f, float mean, Rgb& p) {
#pragma clang fp contract(off)
    const float g = 1.f - f;
    if (code == OP_BRIGHTNESS) {
        p.r = blend(p.r, 0.f, f, g);
        p.g = blend(p.g, 0.f, f, g);
        p.b = blend(p.b, 0.f, f, g);
    } else if (code == OP_CONTRAST) {
        p.r = blend(p.r, mean, f, g);
        p.g = blend(p.g, mean, f, g);
        p.b = blend(p.b, mean, f, g);
    } else if (code == OP_SATURATION) {
        const float y = gray_of(p);
        p.r = blend(p.r, y, f, g);
        p.g = blend(p.g, y, f, g);
        p.b = blend(p.b, y, f, g);
    } else if (code == OP_HUE) {
        hue_shift(p, f);
    }
}

struct Record {
    int code[4];
    float f[4];
};
__device__ __forceinline__ Record load_record(const int8_t* __restrict__ ops, const float* __restrict__ factors, long long t) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(ops + 4 * t);
    const float4 f = *reinterpret_cast<const float4*>(factors + 4 * t);
    Record rec;
#pragma unroll
    for (int k = 0; k < 4; ++k) rec.code[k] = (int)(int8_t)(w >> (8 * k));
    rec.f[0] = f.x; rec.f[1] = f.y; rec.f[2] = f.z; rec.f[3] = f.w;
    return rec;
}

// grid (n_tiles * nblk), kThreads threads: workgroup b of tile t sums the grey values of pixels [b * per, (b + 1) * per) of the tile
__global__ __launch_bounds__(kThreads) void stage_mean_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ tile_img,
                                                              const int32_t* __restrict__ tile_rc, const int8_t* __restrict__ ops,
                                                              const float* __restrict__ factors, int n_tiles, int H, int W, int th, int tw,
                                                              int nblk, void* __restrict__ sums) {
    __shared__ double s_part[kThreads / 64];
    const int t = blockIdx.x / nblk, b = blockIdx.x % nblk, tid = threadIdx.x;
    const Record rec = load_record(ops, factors, t);
    int kc = -1;                                   // the slot of the contrast op
#pragma unroll
    for (int k = 3; k >= 0; --k) kc = rec.code[k] == OP_CONTRAST ? k : kc;
    if (kc < 0) return;                            // uniform: the whole workgroup leaves
    const int npix = th * tw;
    const int per = (npix + nblk - 1) / nblk;
    const int lo = b * per, hi = min(lo + per, npix);
    const uint8_t* img = images + (long long)tile_img[t] * H * W * 3;
    const int r0 = tile_rc[2 * t], c0 = tile_rc[2 * t + 1];
    double acc = 0.0;
    for (int i = lo + tid; i < hi; i += kThreads) {
        const int y = i / tw, x = i - y * tw;
        Rgb p = load_unit(img + ((long long)(r0 + y) * W + (c0 + x)) * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < kc) apply_op(rec.code[k], rec.f[k], 0.f, p);
        acc += (double)gray_of(p);
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) ex_add(sums, n_tiles, 0, t, (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}

template <typename T, bool JITTER>
__global__ __launch_bounds__(kThreads) void stage_apply_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ tile_img,
                                                               const int32_t* __restrict__ tile_rc, const int8_t* __restrict__ flips,
                                                               const int8_t* __restrict__ ops, const float* __restrict__ factors,
                                                               const void* __restrict__ sums, long long n_tiles, int H, int W, int th,
                                                               int tw, float m0, float m1, float m2, float s0, float s1, float s2,
                                                               T* __restrict__ out) {
    const long long npix = (long long)th * tw;
    const long long total = n_tiles * npix;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % tw);
        const int y = (int)((idx / tw) % th);
        const long long t = idx / npix;
        const int flip = flips ? flips[t] : 0;
        const int ys = (flip & 2) ? th - 1 - y : y, xs = (flip & 1) ? tw - 1 - x : x;
        const int r = tile_rc[2 * t] + ys, c = tile_rc[2 * t + 1] + xs;
        const uint8_t* px = images + (((long long)tile_img[t] * H + r) * W + c) * 3;
        Rgb p = load_unit(px);
        if (JITTER) {
            const Record rec = load_record(ops, factors, t);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mean = 0.f;
                if (rec.code[k] == OP_CONTRAST) {
                    if (!sums) continue;           // the caller promised there is none
                    mean = (float)(ex_read(sums, (int)n_tiles, 0, (int)t) / (double)npix);
                }
                apply_op(rec.code[k], rec.f[k], mean, p);
            }
        }
        float v[8];
        // same fp32 operation order as ToTensor + Normalize and tile_gather_kernel: (u8 / 255 - mean) / std
        v[0] = (p.r - m0) / s0;
        v[1] = (p.g - m1) / s1;
        v[2] = (p.b - m2) / s2;
        v[3] = v[4] = v[5] = v[6] = v[7] = 0.f;
        store8<T>(out + idx * 8, v);
    }
}

inline int grid_ew(long long total) {
    long long b = (total + kThreads - 1) / kThreads;
    if (b > 16384) b = 16384;
    if (b < 1) b = 1;
    return (int)b;
}

inline int mean_blocks(long long npix) {
    long long b = (npix + kMeanPixels - 1) / kMeanPixels;
    if (b > kMeanMaxBlocks) b = kMeanMaxBlocks;
    if (b < 1) b = 1;
    return (int)b;
}

template <typename T>
void launch_apply(bool jitter, int grid, hipStream_t st, const uint8_t* images, const int32_t* tile_img, const int32_t* tile_rc,
                  const int8_t* flips, const int8_t* ops, const float* factors, const void* sums, long long n_tiles, int H, int W, int th,
                  int tw, const float* m, const float* s, T* out) {
    if (jitter)
        hipLaunchKernelGGL((stage_apply_kernel<T, true>), dim3(grid), dim3(kThreads), 0, st, images, tile_img, tile_rc, flips, ops, factors,
                           sums, n_tiles, H, W, th, tw, m[0], m[1], m[2], s[0], s[1], s[2], out);
    else
        hipLaunchKernelGGL((stage_apply_kernel<T, false>), dim3(grid), dim3(kThreads), 0, st, images, tile_img, tile_rc, flips, ops, factors,
                           sums, n_tiles, H, W, th, tw, m[0], m[1], m[2], s[0], s[1], s[2], out);
}

}  // namespace

// workspace: the exact-limb accumulator of one grey sum per tile (ex_words(T) 8-byte words), zeroed by the call itself
extern "C" size_t cs_stage_augmented_workspace(long long n_tiles) {
    if (n_tiles <= 0 || n_tiles > INT_MAX) return 0;
    return (size_t)ex_words((int)n_tiles) * 8;
}

extern "C" int cs_stage_augmented(const uint8_t* images, int n_images, int H, int W, const int32_t* tile_img, const int32_t* tile_rc,
                                  const int8_t* flips, const int8_t* jitter_ops, const float* jitter_factors, int has_contrast,
                                  long long n_tiles, int th, int tw, const float* host_mean3, const float* host_std3, int dtype, void* out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(images && tile_img && tile_rc && out && host_mean3 && host_std3, "stage_augmented: NULL argument");
    CS_CHECK_ARG((jitter_ops != nullptr) == (jitter_factors != nullptr), "stage_augmented: jitter op codes and factors come together");
    CS_CHECK_ARG(n_images > 0 && H > 0 && W > 0 && n_tiles > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "stage_augmented: bad extents");
    CS_CHECK_ARG(n_tiles <= INT_MAX && (long long)th * tw <= INT_MAX, "stage_augmented: 2^31 tiles, or pixels in a tile, or more");
    CS_CHECK_ARG(dtype == CS_F32 || dtype == CS_BF16, "stage_augmented: bad dtype");
    CS_CHECK_ARG(has_contrast == 0 || has_contrast == 1, "stage_augmented: has_contrast is 0 or 1");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(jitter_ops) & 3) == 0 && (reinterpret_cast<uintptr_t>(jitter_factors) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(out) & 15) == 0, "stage_augmented: misaligned argument");
    const int nblk = mean_blocks((long long)th * tw);
    if (has_contrast) {
        CS_CHECK_ARG(jitter_ops, "stage_augmented: has_contrast without a jitter record");
        CS_CHECK_ARG(n_tiles * nblk <= INT_MAX, "stage_augmented: 2^31 reduction workgroups or more");
        CS_CHECK_ARG(workspace && workspace_bytes >= cs_stage_augmented_workspace(n_tiles), "stage_augmented: workspace too small");
        CS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "stage_augmented: misaligned workspace");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const void* sums = nullptr;
    if (has_contrast) {
        if (hipMemsetAsync(workspace, 0, cs_stage_augmented_workspace(n_tiles), st) != hipSuccess) {
            cs_set_error_("stage_augmented: memset failed");
            return CS_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(stage_mean_kernel, dim3((unsigned)(n_tiles * nblk)), dim3(kThreads), 0, st, images, tile_img, tile_rc, jitter_ops,
                           jitter_factors, (int)n_tiles, H, W, th, tw, nblk, workspace);
        CS_LAUNCH_CHECK();
        sums = workspace;
    }
    const int grid = grid_ew(n_tiles * th * tw);
    if (dtype == CS_F32)
        launch_apply<float>(jitter_ops != nullptr, grid, st, images, tile_img, tile_rc, flips, jitter_ops, jitter_factors, sums, n_tiles, H, W,
                            th, tw, host_mean3, host_std3, (float*)out);
    else
        launch_apply<bf16_t>(jitter_ops != nullptr, grid, st, images, tile_img, tile_rc, flips, jitter_ops, jitter_factors, sums, n_tiles, H, W,
                             th, tw, host_mean3, host_std3, (bf16_t*)out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
