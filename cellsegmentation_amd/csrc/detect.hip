// Cell localisation from segmentation probability maps (test_seg.py `meanshift_cluster` / `cell_detect`, --detect path):
//   quantise  u8 = trunc(255 p) in fp32
//   blur      separable integer Gaussian, taps summing to 2^14, BORDER_REFLECT_101, int32 row pass / int64 column pass,
//             out = (s + 2^27) >> 28
//   seeds     the get_tiles(interval, window) grid, kept where blurred[centre] > thr * 255 (fp64)
//   meanshift cv2.meanShift with TermCriteria(EPS, 0, 1e-5): up to max_iter steps of dx = rint(m10 / m00 - ws / 2) (fp64),
//             clamped to the image; a step that does not move the window is a fixed point, so the loop stops there
//   cluster   DBSCAN(eps, min_samples=1): connected components of dr^2 + dc^2 <= eps^2; root = lowest point index
//   centroids rint(sum / n) of exact integer sums; weight = blurred[centroid]; order: weight desc, label desc
//   stitch    patches written into a zeroed whole-image mask, the highest patch index winning where patches overlap
//   streamed  the same mask built batch by batch: softmax channel + quantise of a batch of logits written in place in one launch,
//             the owner of a pixel decided from the batch's corners (no per-pixel state); earlier batches are overwritten in stream order
//   blended   overlaps averaged instead of overwritten: per pixel the integer sums of w * level and of w over every covering patch
//             (flipped views included), mask = floor(sum / (256 sum of w)); the lowest covering index of a batch owns the update
//   distance  method="distancetransform" puts the exact distance transform of morph.hip in the blur's place; the rest is unchanged
// Every step is integer arithmetic or one correctly rounded fp64 operation, so the result does not depend on launch order.
#include "cs_common.h"
#include "cs_block.h"
#include "cs_softmax.h"

namespace {

constexpr int kMaxHalf = 15;          // ksize <= 31
constexpr int kBT = 64;               // blur output tile: kBT x kBT pixels per 256-thread workgroup
constexpr int kBIn = kBT + 2 * kMaxHalf;
constexpr int kMsLdsBytes = 96 * 1024;  // maps up to this many pixels are staged whole in LDS by the mean-shift kernel
constexpr int kLdsPts = 2048;         // clustering within one workgroup up to this many points per image
constexpr int kMaxWindow = 128;       // moments of a window stay below 2^31

struct Taps {
    int32_t t[2 * kMaxHalf + 1];
};

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__global__ __launch_bounds__(256) void quantize_kernel(const float* __restrict__ p, long long n, uint8_t* __restrict__ out) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(p)[i];
        const uint32_t o = (uint32_t)quant(v.x) | ((uint32_t)quant(v.y) << 8) | ((uint32_t)quant(v.z) << 16) | ((uint32_t)quant(v.w) << 24);
        reinterpret_cast<uint32_t*>(out)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[n4 * 4 + threadIdx.x] = quant(p[n4 * 4 + threadIdx.x]);
}

// One workgroup per 64 x 64 output tile of one image.  The (64 + 2 hy) x (64 + 2 hx) source window is staged in LDS as u8
// (quantised on the way in when the source is fp32), the row pass writes int32 sums to LDS, the column pass accumulates int64.
template <bool F32>
__global__ __launch_bounds__(256) void blur_kernel(const void* __restrict__ src, int H, int W, Taps tx, int hx, Taps ty, int hy,
                                                   uint8_t* __restrict__ dst) {
    __shared__ uint8_t in[kBIn][kBIn + 2];
    __shared__ int32_t rs[kBIn][kBT];
    const int c0 = blockIdx.x * kBT, r0 = blockIdx.y * kBT;
    const long long img = (long long)blockIdx.z * H * W;
    const int rows = kBT + 2 * hy, cols = kBT + 2 * hx;
    constexpr int V = F32 ? 4 : 16;                     // elements per 16-byte load
    const bool vec = c0 + kBT <= W && (W % V) == 0;
    const float* sf = reinterpret_cast<const float*>(src) + img;
    const uint8_t* su = reinterpret_cast<const uint8_t*>(src) + img;
    auto fetch = [&](long long off) -> uint8_t { return F32 ? quant(sf[off]) : su[off]; };
    if (vec) {
        // central 64 columns: 16-byte loads
        constexpr int per_row = kBT / V;
        for (int e = threadIdx.x; e < rows * per_row; e += 256) {
            const int rr = e / per_row, ch = e - rr * per_row;
            const long long off = (long long)reflect101(r0 - hy + rr, H) * W + c0 + ch * V;
            uint8_t* d = &in[rr][hx + ch * V];
            if (F32) {
                const float4 v = *reinterpret_cast<const float4*>(sf + off);
                d[0] = quant(v.x); d[1] = quant(v.y); d[2] = quant(v.z); d[3] = quant(v.w);
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(su + off);
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 16; ++q) d[q] = (uint8_t)(w4[q >> 2] >> ((q & 3) * 8));
            }
        }
        // halo columns
        for (int e = threadIdx.x; e < rows * 2 * hx; e += 256) {
            const int rr = e / (2 * hx), k = e - rr * 2 * hx;
            const int cc = k < hx ? k : kBT + k;
            in[rr][cc] = fetch((long long)reflect101(r0 - hy + rr, H) * W + reflect101(c0 - hx + cc, W));
        }
    } else {
        for (int e = threadIdx.x; e < rows * cols; e += 256) {
            const int rr = e / cols, cc = e - rr * cols;
            in[rr][cc] = fetch((long long)reflect101(r0 - hy + rr, H) * W + reflect101(c0 - hx + cc, W));
        }
    }
    __syncthreads();
    const int kx = 2 * hx + 1, ky = 2 * hy + 1;
    for (int e = threadIdx.x; e < rows * kBT; e += 256) {
        const int rr = e / kBT, c = e - rr * kBT;
        int32_t s = 0;
        for (int i = 0; i < kx; ++i) s += tx.t[i] * (int32_t)in[rr][c + i];
        rs[rr][c] = s;
    }
    __syncthreads();
    // 16 consecutive output pixels per thread: one 16-byte store
    const int r = threadIdx.x >> 2, cb = (threadIdx.x & 3) * 16;
    const int gr = r0 + r;
    if (gr >= H) return;
    uint8_t o[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        long long s = 0;
        for (int j = 0; j < ky; ++j) s += (long long)ty.t[j] * rs[r + j][cb + q];
        o[q] = (uint8_t)((s + (1LL << 27)) >> 28);
    }
    uint8_t* d = dst + img + (long long)gr * W + c0 + cb;
    if (c0 + cb + 16 <= W && (W % 16) == 0) {
        uint4 v;
        v.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
        v.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
        v.z = o[8] | (o[9] << 8) | (o[10] << 16) | ((uint32_t)o[11] << 24);
        v.w = o[12] | (o[13] << 8) | (o[14] << 16) | ((uint32_t)o[15] << 24);
        *reinterpret_cast<uint4*>(d) = v;
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (c0 + cb + q < W) d[q] = o[q];
    }
}

// ---- stitching: the highest patch index covering a pixel owns it --------------------------------------------------------------
__global__ __launch_bounds__(256) void stitch_init_kernel(int32_t* __restrict__ owner, long long HW) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) owner[i] = -1;
}
__global__ __launch_bounds__(256) void stitch_claim_kernel(const int32_t* __restrict__ corners, int ph, int pw, int H, int W,
                                                           int32_t* __restrict__ owner) {
    const int m = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ph * pw) return;
    const int r = corners[2 * m] + e / pw, c = corners[2 * m + 1] + e % pw;
    if (r >= 0 && r < H && c >= 0 && c < W) atomicMax(owner + (long long)r * W + c, m);
}
__global__ __launch_bounds__(256) void stitch_gather_kernel(const uint8_t* __restrict__ patches, const int32_t* __restrict__ corners,
                                                            int ph, int pw, int H, int W, const int32_t* __restrict__ owner,
                                                            uint8_t* __restrict__ out) {
    const long long HW = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        const int m = owner[i];
        uint8_t v = 0;
        if (m >= 0) {
            const int r = (int)(i / W), c = (int)(i % W);
            v = patches[((long long)m * ph + (r - corners[2 * m])) * pw + (c - corners[2 * m + 1])];
        }
        out[i] = v;
    }
}

// ---- streamed stitching: a batch of segment logits written straight into the whole-image mask ---------------------------------
// bits [lo, hi) of a four-pixel unit (either end may lie outside 0..4)
__device__ __forceinline__ uint32_t unit_bits(int lo, int hi) {
    lo = min(max(lo, 0), 4);
    hi = min(max(hi, 0), 4);
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// mask[R][Cc] = quant(softmax over the channels of logits[b], channel ch) for every pixel of every patch b that no later patch of the
// batch covers.  Ownership comes from the corners alone: a workgroup-uniform walk over the later corners skips the rectangles that
// lie apart from patch b, the others cost a row test and a column interval per lane.  So a mask byte is written at most once per
// launch, without atomics and whatever order the workgroups run in; bytes that no patch covers are not touched.
// A workgroup takes 256 units of one patch at a time.  A unit is the four mask bytes of one aligned dword of a patch row (ng units
// span a row at any alignment): a wholly owned unit is one dword store, a patch edge or a partly covered unit is byte stores.
__global__ __launch_bounds__(256) void stitch_logits_kernel(const float* __restrict__ logits, const int32_t* __restrict__ corners, int B, int C,
                                                            int ch, int ph, int pw, int H, int W, int ng, int chunks,
                                                            uint8_t* __restrict__ mask) {
    const long long items = (long long)B * chunks, plane = (long long)ph * pw;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / chunks);
        const int u = (int)(item - (long long)b * chunks) * 256 + threadIdx.x;
        const long long r0 = corners[2 * b], c0 = corners[2 * b + 1];
        if (r0 >= H || r0 + ph <= 0 || c0 >= W || c0 + pw <= 0) continue;          // workgroup-uniform: the patch misses the mask
        const int r = u / ng, g = u - r * ng;
        const int R = (int)r0 + r;
        if (r >= ph || R < 0 || R >= H) continue;
        const long long row = (long long)R * W;
        const int lead = (int)((reinterpret_cast<uintptr_t>(mask) + row + c0) & 3);   // bytes between the dword boundary and the patch row
        const int p0 = 4 * g - lead, C0 = (int)c0 + p0;                              // the unit's first column in the patch / in the mask
        uint32_t want = unit_bits(max(-p0, -C0), min(pw - p0, W - C0));              // inside the patch and inside the mask
        if (!want) continue;
        for (int m = b + 1; m < B; ++m) {
            const long long mr = corners[2 * m], mc = corners[2 * m + 1];
            if (mr >= r0 + ph || mr + ph <= r0 || mc >= c0 + pw || mc + pw <= c0) continue;      // workgroup-uniform: rectangles apart
            if ((unsigned)(R - (int)mr) < (unsigned)ph) want &= ~unit_bits((int)mc - C0, (int)mc + pw - C0);
        }
        if (!want) continue;
        const long long src = ((long long)b * C * ph + r) * pw + p0;                 // channel 0 of the unit's first pixel
        const long long dst = row + C0;                                               // 64-bit: a slide mask may exceed 2^31 pixels
        if (want == 0xfu) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) o |= (uint32_t)quant(softmax_channel_at(logits + (src + j), plane, C, ch)) << (8 * j);
            *reinterpret_cast<uint32_t*>(mask + dst) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((want >> j) & 1u) mask[dst + j] = quant(softmax_channel_at(logits + (src + j), plane, C, ch));
        }
    }
}

// ---- blended stitching: every patch that covers a pixel adds its weighted level to two whole-image accumulators ------------------
// The level of a probability: quant()'s clamp, then 256 steps per mask level.  The product by 256 is exact in fp32, so
// blend_level(p) >> 8 == quant(p); a NaN gives 0, as in quant.
__device__ __forceinline__ uint32_t blend_level(float p) {
    const float v = fminf(fmaxf(255.0f * p, 0.f), 255.f);
    return (uint32_t)(256.0f * v);
}

// num[R][Cc] += sum of w q, den[R][Cc] += sum of w over the patches m of the batch that cover slide pixel (R, Cc): q = blend_level of
// the softmax of patch m at that pixel, w = tr[i] tc[j] with (i, j) the pixel's position inside patch m ON THE SLIDE.  flips[m]
// (1 horizontal, 2 vertical, 3 both) says that logits[m] are those of the flipped tile: slide position (i, j) reads logit pixel
// (ph-1-i if code & 2 else i, pw-1-j if code & 1 else j).
// Ownership comes from the corners alone, as in stitch_logits_kernel, with the LOWEST covering index as the owner: a
// workgroup-uniform walk over the earlier corners strips the pixels that an earlier patch covers, a second walk over the patches
// from b on sums every contribution in registers, and the owner does one plain read-modify-write.  So an accumulator element is
// updated at most once per launch, without atomics and whatever order the workgroups run in; integer sums make the result
// independent of how the patches are split into launches.  Units are four slide pixels at a 4-element boundary of the
// accumulators (16 bytes of den, 32 of num): a wholly owned unit is vector loads and stores, the rest element by element.
__global__ __launch_bounds__(256) void stitch_blend_add_kernel(const float* __restrict__ logits, const int32_t* __restrict__ corners,
                                                               const uint8_t* __restrict__ flips, const int32_t* __restrict__ tr,
                                                               const int32_t* __restrict__ tc, int B, int C, int ch, int ph, int pw, int H,
                                                               int W, int ng, int chunks, unsigned long long* __restrict__ num,
                                                               uint32_t* __restrict__ den) {
    const long long items = (long long)B * chunks, plane = (long long)ph * pw;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / chunks);
        const int u = (int)(item - (long long)b * chunks) * 256 + threadIdx.x;
        const long long r0 = corners[2 * b], c0 = corners[2 * b + 1];
        if (r0 >= H || r0 + ph <= 0 || c0 >= W || c0 + pw <= 0) continue;          // workgroup-uniform: the patch misses the slide
        const int r = u / ng, g = u - r * ng;
        const int R = (int)r0 + r;
        if (r >= ph || R < 0 || R >= H) continue;
        const long long row = (long long)R * W;
        const int lead = (int)((row + c0) & 3);                                      // elements between the unit boundary and the patch row
        const int p0 = 4 * g - lead, C0 = (int)c0 + p0;                              // the unit's first column in the patch / on the slide
        uint32_t want = unit_bits(max(-p0, -C0), min(pw - p0, W - C0));              // inside the patch and inside the slide
        if (!want) continue;
        for (int m = 0; m < b; ++m) {                                                // an earlier patch that covers a pixel owns it
            const long long mr = corners[2 * m], mc = corners[2 * m + 1];
            if (mr >= r0 + ph || mr + ph <= r0 || mc >= c0 + pw || mc + pw <= c0) continue;      // workgroup-uniform: rectangles apart
            if ((unsigned)(R - (int)mr) < (unsigned)ph) want &= ~unit_bits((int)mc - C0, (int)mc + pw - C0);
        }
        if (!want) continue;
        unsigned long long sn[4] = {0, 0, 0, 0};
        uint32_t sd[4] = {0, 0, 0, 0};
        for (int m = b; m < B; ++m) {                                                // patch b itself, then the later ones that reach it
            const long long mr = corners[2 * m], mc = corners[2 * m + 1];
            if (mr >= r0 + ph || mr + ph <= r0 || mc >= c0 + pw || mc + pw <= c0) continue;      // workgroup-uniform
            const int i = R - (int)mr;
            if ((unsigned)i >= (unsigned)ph) continue;
            const uint32_t cover = want & unit_bits((int)mc - C0, (int)mc + pw - C0);
            if (!cover) continue;
            const int code = flips ? flips[m] : 0;
            const long long base = ((long long)m * C * ph + ((code & 2) ? ph - 1 - i : i)) * pw;     // channel 0 of the logit row
            const uint32_t wr = (uint32_t)tr[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((cover >> j) & 1u)) continue;
                const int jj = C0 + j - (int)mc;
                const uint32_t w = wr * (uint32_t)tc[jj];
                const uint32_t q = blend_level(softmax_channel_at(logits + (base + ((code & 1) ? pw - 1 - jj : jj)), plane, C, ch));
                sn[j] += (unsigned long long)w * q;
                sd[j] += w;
            }
        }
        const long long dst = row + C0;                                               // 64-bit: a slide may exceed 2^31 pixels
        if (want == 0xfu) {
            ulonglong2* n2 = reinterpret_cast<ulonglong2*>(num + dst);
            uint4* d4 = reinterpret_cast<uint4*>(den + dst);
            ulonglong2 lo = n2[0], hi = n2[1];
            uint4 d = *d4;
            lo.x += sn[0]; lo.y += sn[1]; hi.x += sn[2]; hi.y += sn[3];
            d.x += sd[0]; d.y += sd[1]; d.z += sd[2]; d.w += sd[3];
            n2[0] = lo; n2[1] = hi;
            *d4 = d;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((want >> j) & 1u) {
                    num[dst + j] += sn[j];
                    den[dst + j] += sd[j];
                }
        }
    }
}

// mask = den ? floor(num / (256 den)) : 0.  num <= 255 * 256 * den for sums that stitch_blend_add_kernel made, so the byte holds it.
__device__ __forceinline__ uint32_t blend_byte(unsigned long long n, uint32_t d) {
    return d ? (uint32_t)(n / (256ull * d)) & 0xffu : 0u;
}
// n4 four-pixel units with vector loads and one dword store (0 when a buffer is not aligned for them), the rest element by element.
__global__ __launch_bounds__(256) void stitch_blend_finish_kernel(const unsigned long long* __restrict__ num, const uint32_t* __restrict__ den,
                                                                  long long n, long long n4, uint8_t* __restrict__ mask) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long i = t; i < n4; i += step) {
        const ulonglong2 lo = reinterpret_cast<const ulonglong2*>(num)[2 * i], hi = reinterpret_cast<const ulonglong2*>(num)[2 * i + 1];
        const uint4 d = reinterpret_cast<const uint4*>(den)[i];
        reinterpret_cast<uint32_t*>(mask)[i] =
            blend_byte(lo.x, d.x) | (blend_byte(lo.y, d.y) << 8) | (blend_byte(hi.x, d.z) << 16) | (blend_byte(hi.y, d.w) << 24);
    }
    for (long long i = 4 * n4 + t; i < n; i += step) mask[i] = (uint8_t)blend_byte(num[i], den[i]);
}

// ---- seeds + mean shift -------------------------------------------------------------------------------------------------------
struct Grid {
    int nr, nc;          // origins per axis
    int n0r, n0c;        // regular origins (k * interval) per axis; a last border-aligned origin follows when n0 < n
    int interval, window, H, W;
};
__host__ __device__ inline int axis_count(int len, int interval, int size, int* n0) {
    const int a = (len - size) / interval + 1;
    *n0 = a;
    return (a - 1) * interval + size == len ? a : a + 1;
}
__device__ __forceinline__ int axis_origin(int k, int n0, int len, int interval, int size) {
    return k < n0 ? k * interval : len - size;
}

// One workgroup per image: keep the grid windows whose blurred centre is above thr255 and write their corners, in grid order, to
// pts[n][0..count) (the mean-shift kernels move them in place).
__global__ __launch_bounds__(1024) void seed_kernel(const uint8_t* __restrict__ blurred, Grid g, double thr255, int32_t* __restrict__ pts,
                                                    int32_t* __restrict__ n_pts) {
    __shared__ int wsum[16];
    const int G = g.nr * g.nc;
    const uint8_t* img = blurred + (long long)blockIdx.x * g.H * g.W;
    int32_t* out = pts + (long long)blockIdx.x * G * 2;
    const int half = g.window / 2;
    int carry = 0;
    for (int base = 0; base < G; base += 1024) {
        const int k = base + threadIdx.x;
        int r = 0, c = 0, keep = 0;
        if (k < G) {
            r = axis_origin(k / g.nc, g.n0r, g.H, g.interval, g.window);
            c = axis_origin(k % g.nc, g.n0c, g.W, g.interval, g.window);
            keep = (double)img[(long long)(r + half) * g.W + c + half] > thr255;
        }
        int total;
        const int at = carry + block_rank<1024>(keep, wsum, total);
        if (keep) {
            out[2 * at] = r;
            out[2 * at + 1] = c;
        }
        carry += total;
    }
    if (threadIdx.x == 0) n_pts[blockIdx.x] = carry;
}

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wave: cv2.meanShift of the window at corner (r, c) over img (row stride W; LDS or global); returns the final corner.
__device__ __forceinline__ void meanshift_window(const uint8_t* img, int H, int W, int ws, int max_iter, int& r, int& c) {
    const int lane = threadIdx.x & 63;
    const double half = 0.5 * ws;
    for (int it = 0; it < max_iter; ++it) {
        int m00 = 0, m10 = 0, m01 = 0;
        for (int e = lane; e < ws * ws; e += 64) {
            const int y = e / ws, x = e - y * ws;
            const int v = img[(long long)(r + y) * W + c + x];
            m00 += v;
            m10 += x * v;
            m01 += y * v;
        }
        m00 = wave_isum(m00);
        m10 = wave_isum(m10);
        m01 = wave_isum(m01);
        if (m00 == 0) break;                                   // wave-uniform: every lane holds the reduced moments
        const int dx = (int)rint((double)m10 / (double)m00 - half);
        const int dy = (int)rint((double)m01 / (double)m00 - half);
        const int nc = min(max(c + dx, 0), W - ws);
        const int nr = min(max(r + dy, 0), H - ws);
        if (nc == c && nr == r) break;                         // fixed point: the remaining iterations change nothing
        c = nc;
        r = nr;
    }
}

// Maps of at most kMsLdsBytes pixels: one workgroup per image stages the whole blurred map in LDS, its 16 waves take the image's
// windows in turn.
__global__ __launch_bounds__(1024) void meanshift_lds_kernel(const uint8_t* __restrict__ blurred, int H, int W, int G, int ws, int max_iter,
                                                             int32_t* __restrict__ pts, const int32_t* __restrict__ n_pts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char img[];
    const long long HW = (long long)H * W;
    const uint8_t* src = blurred + blockIdx.x * HW;
    if ((HW & 15) == 0) {
        for (long long i = threadIdx.x; i < HW / 16; i += 1024) reinterpret_cast<uint4*>(img)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else {
        for (long long i = threadIdx.x; i < HW; i += 1024) img[i] = src[i];
    }
    __syncthreads();
    const int n = n_pts[blockIdx.x];
    int32_t* p = pts + (long long)blockIdx.x * G * 2;
    const int half = ws / 2;
    for (int k = threadIdx.x >> 6; k < n; k += 16) {
        int r = p[2 * k], c = p[2 * k + 1];
        meanshift_window(img, H, W, ws, max_iter, r, c);
        if ((threadIdx.x & 63) == 0) {
            p[2 * k] = r + half;
            p[2 * k + 1] = c + half;
        }
    }
}

// Larger maps: one wave per window, moments read from global memory.
__global__ __launch_bounds__(256) void meanshift_global_kernel(const uint8_t* __restrict__ blurred, int N, int H, int W, int G, int ws, int max_iter,
                                                               int32_t* __restrict__ pts, const int32_t* __restrict__ n_pts) {
    const long long wi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wi >= (long long)N * G) return;
    const int n = (int)(wi / G), k = (int)(wi % G);
    if (k >= n_pts[n]) return;
    int32_t* p = pts + ((long long)n * G + k) * 2;
    int r = p[0], c = p[1];
    meanshift_window(blurred + (long long)n * H * W, H, W, ws, max_iter, r, c);
    if ((threadIdx.x & 63) == 0) {
        p[0] = r + ws / 2;
        p[1] = c + ws / 2;
    }
}

// ---- clustering -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool linked(int ar, int ac, int br, int bc, double eps2) {
    const long long dr = ar - br, dc = ac - bc;
    return (double)(dr * dr + dc * dc) <= eps2;
}

// Points of one image in one workgroup: hook the larger root of every linked pair to the smaller (LDS atomicMin), compress every
// path to its root, repeat until a round hooks nothing.  Labels only decrease and every root is the lowest index of its tree,
// so the result is the lowest index of each component whatever order the hooks land in.
__global__ __launch_bounds__(1024) void cluster_lds_kernel(const int32_t* __restrict__ pts, const int32_t* __restrict__ n_pts, int cap,
                                                           double eps2, int32_t* __restrict__ lab_out) {
    __shared__ int pr[kLdsPts], pc[kLdsPts], lab[kLdsPts];
    __shared__ int changed;
    const int n = min(n_pts[blockIdx.x], cap);
    const int32_t* p = pts + (long long)blockIdx.x * cap * 2;
    for (int i = threadIdx.x; i < n; i += 1024) {
        pr[i] = p[2 * i];
        pc[i] = p[2 * i + 1];
        lab[i] = i;
    }
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    for (;;) {
        bool hooked = false;
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int ir = pr[i], ic = pc[i];
            for (int j = i + 1; j < n; ++j) {
                if (!linked(ir, ic, pr[j], pc[j], eps2)) continue;
                const int a = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i), b = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, j);
                if (a != b) {
                    atomicMin(&lab[max(a, b)], min(a, b));
                    hooked = true;
                }
            }
        }
        if (hooked) changed = 1;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i);
            __hip_atomic_store(&lab[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        const int ch = changed;
        __syncthreads();
        if (!ch) break;
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += 1024) lab_out[(long long)blockIdx.x * cap + i] = lab[i];
}

// Global form of the same rounds, one launch per phase: no workgroup reads what another workgroup of the same launch wrote
// except through the hooks themselves, whose order does not matter (every label value ever held is an ancestor).
// state[0]: a hook landed in this round; state[1]: a round without hooks has been seen (later launches return at once).
__global__ __launch_bounds__(256) void cluster_init_kernel(const int32_t* __restrict__ n_pts, int N, int cap, int32_t* __restrict__ lab,
                                                           int32_t* __restrict__ state) {
    const long long total = (long long)N * cap;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) lab[i] = (int)(i % cap);
    if (blockIdx.x == 0 && threadIdx.x < 2) state[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void cluster_hook_kernel(const int32_t* __restrict__ pts, const int32_t* __restrict__ n_pts, int cap,
                                                           double eps2, int32_t* __restrict__ lab_all, int32_t* __restrict__ state) {
    const int ib = blockIdx.x, jb = blockIdx.y, img = blockIdx.z;
    if (jb < ib) return;
    if (__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const int n = min(n_pts[img], cap);
    if (ib * 256 >= n || jb * 256 >= n) return;
    const int32_t* p = pts + (long long)img * cap * 2;
    int32_t* lab = lab_all + (long long)img * cap;
    __shared__ int tr[256], tc[256];
    __shared__ int any;
    const int j0 = jb * 256;
    if (j0 + (int)threadIdx.x < n) {
        tr[threadIdx.x] = p[2 * (j0 + threadIdx.x)];
        tc[threadIdx.x] = p[2 * (j0 + threadIdx.x) + 1];
    }
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    const int i = ib * 256 + threadIdx.x;
    bool hooked = false;
    if (i < n) {
        const int ir = p[2 * i], ic = p[2 * i + 1];
        const int jn = min(256, n - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const int j = j0 + jj;
            if (j <= i || !linked(ir, ic, tr[jj], tc[jj], eps2)) continue;
            const int a = uf_find<__HIP_MEMORY_SCOPE_AGENT>(lab, i), b = uf_find<__HIP_MEMORY_SCOPE_AGENT>(lab, j);
            if (a != b) {
                __hip_atomic_fetch_min(lab + max(a, b), min(a, b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                hooked = true;
            }
        }
    }
    if (hooked) any = 1;
    __syncthreads();
    if (threadIdx.x == 0 && any) __hip_atomic_store(state, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void cluster_jump_kernel(const int32_t* __restrict__ n_pts, int N, int cap, int32_t* __restrict__ lab_all,
                                                           const int32_t* __restrict__ state) {
    if (__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const long long total = (long long)N * cap;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int img = (int)(g / cap), i = (int)(g % cap);
        if (i >= min(n_pts[img], cap)) continue;
        int32_t* lab = lab_all + (long long)img * cap;
        __hip_atomic_store(lab + i, uf_find<__HIP_MEMORY_SCOPE_AGENT>(lab, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void cluster_round_end_kernel(int32_t* __restrict__ state) {
    if (state[1]) return;
    if (!state[0]) state[1] = 1;
    state[0] = 0;
}

// One workgroup per image: cluster number of every root = number of roots before it (DBSCAN's labels); per-cluster sums zeroed.
__global__ __launch_bounds__(1024) void cluster_ids_kernel(const int32_t* __restrict__ n_pts, int cap, const int32_t* __restrict__ lab_all,
                                                           int32_t* __restrict__ cid_all, int32_t* __restrict__ n_clu,
                                                           unsigned long long* __restrict__ sums) {
    __shared__ int wsum[16];
    const int n = min(n_pts[blockIdx.x], cap);
    const int32_t* lab = lab_all + (long long)blockIdx.x * cap;
    int32_t* cid = cid_all + (long long)blockIdx.x * cap;
    int nc = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const bool is_root = i < n && lab[i] == i;
        int total;
        const int before = block_rank<1024>(is_root, wsum, total);
        if (is_root) cid[i] = nc + before;
        nc += total;
    }
    unsigned long long* s = sums + (long long)blockIdx.x * cap * 3;
    for (int k = threadIdx.x; k < 3 * nc; k += 1024) s[k] = 0;
    if (threadIdx.x == 0) n_clu[blockIdx.x] = nc;
}

__global__ __launch_bounds__(256) void cluster_accum_kernel(const int32_t* __restrict__ pts, const int32_t* __restrict__ n_pts, int N, int cap,
                                                            const int32_t* __restrict__ lab_all, const int32_t* __restrict__ cid_all,
                                                            unsigned long long* __restrict__ sums) {
    const long long total = (long long)N * cap;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int img = (int)(g / cap), i = (int)(g % cap);
        if (i >= min(n_pts[img], cap)) continue;
        const long long base = (long long)img * cap;
        const int k = cid_all[base + lab_all[g]];
        unsigned long long* s = sums + (base + k) * 3;
        atomicAdd(s, (unsigned long long)pts[2 * g]);
        atomicAdd(s + 1, (unsigned long long)pts[2 * g + 1]);
        atomicAdd(s + 2, 1ull);
    }
}

// single workgroup: off[0] = 0, off[i + 1] = off[i] + n_clu[i]
__global__ __launch_bounds__(256) void cluster_offsets_kernel(const int32_t* __restrict__ n_clu, int N, int64_t* __restrict__ off) {
    __shared__ long long part[256];
    long long carry = 0, total;
    if (threadIdx.x == 0) off[0] = 0;
    for (int b0 = 0; b0 < N; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const long long incl = block_scan_incl<256, long long>(i < N ? n_clu[i] : 0, part, total);
        if (i < N) off[i + 1] = carry + incl;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void cluster_centroid_kernel(const int32_t* __restrict__ n_clu, int N, int cap,
                                                               const unsigned long long* __restrict__ sums, const int64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ blurred, int H, int W, float* __restrict__ key,
                                                               int32_t* __restrict__ cent, int32_t* __restrict__ wgt) {
    const long long total = (long long)N * cap;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int img = (int)(g / cap), k = (int)(g % cap);
        if (k >= n_clu[img]) continue;
        const unsigned long long* s = sums + g * 3;
        const double cnt = (double)s[2];
        const int cr = min(max((int)rint((double)s[0] / cnt), 0), H - 1);
        const int cc = min(max((int)rint((double)s[1] / cnt), 0), W - 1);
        const int w = blurred[((long long)img * H + cr) * W + cc];
        const long long pos = off[img] + k;
        key[pos] = (float)w;
        cent[2 * pos] = cr;
        cent[2 * pos + 1] = cc;
        wgt[pos] = w;
    }
}

// order = stable ascending (weight, label) per image; emit it reversed: weight descending, label descending
__global__ __launch_bounds__(256) void cluster_emit_kernel(const int32_t* __restrict__ n_clu, int N, int cap, const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ order, const int32_t* __restrict__ cent,
                                                           const int32_t* __restrict__ wgt, int64_t* __restrict__ out_pts,
                                                           int32_t* __restrict__ out_w) {
    const long long total = (long long)N * cap;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int img = (int)(g / cap), k = (int)(g % cap);
        const int n = n_clu[img];
        if (k >= n) continue;
        const long long pos = off[img] + k;
        const long long src = order[off[img] + (n - 1 - k)];
        out_pts[2 * pos] = cent[2 * src];
        out_pts[2 * pos + 1] = cent[2 * src + 1];
        out_w[pos] = wgt[src];
    }
}

inline unsigned grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b < 1) b = 1;
    return (unsigned)(b > 8192 ? 8192 : b);
}

bool taps_ok(const int32_t* t, int k) {
    if (!t || k < 1 || k > 2 * kMaxHalf + 1 || (k & 1) == 0) return false;
    long long s = 0;
    for (int i = 0; i < k; ++i) {
        if (t[i] < 0) return false;
        s += t[i];
    }
    return s == (1 << 14);
}

}  // namespace

extern "C" int cs_detect_quantize(const float* probs, long long n, uint8_t* out, void* stream) {
    CS_CHECK_ARG(probs && out && n > 0, "detect_quantize: bad arguments");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(probs) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                 "detect_quantize: misaligned buffers");
    hipLaunchKernelGGL(quantize_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), probs, n, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_detect_blur(const void* src, int src_is_f32, int N, int H, int W, const int32_t* taps_x, int kx, const int32_t* taps_y,
                              int ky, uint8_t* dst, void* stream) {
    CS_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0, "detect_blur: bad arguments");
    CS_CHECK_ARG(taps_ok(taps_x, kx) && taps_ok(taps_y, ky), "detect_blur: taps must be an odd count <= 31 of non-negative integers summing to 2^14");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0, "detect_blur: misaligned buffers");
    CS_CHECK_ARG(N <= 65535, "detect_blur: too many images in one call");
    Taps tx{}, ty{};
    for (int i = 0; i < kx; ++i) tx.t[i] = taps_x[i];
    for (int i = 0; i < ky; ++i) ty.t[i] = taps_y[i];
    const dim3 grid(cs_ceil_div(W, kBT), cs_ceil_div(H, kBT), N);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (src_is_f32)
        hipLaunchKernelGGL(blur_kernel<true>, grid, dim3(256), 0, st, src, H, W, tx, kx / 2, ty, ky / 2, dst);
    else
        hipLaunchKernelGGL(blur_kernel<false>, grid, dim3(256), 0, st, src, H, W, tx, kx / 2, ty, ky / 2, dst);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_stitch_workspace(int H, int W) { return (size_t)H * W * sizeof(int32_t); }

extern "C" int cs_stitch_patches(const uint8_t* patches, int M, int ph, int pw, const int32_t* corners, int H, int W, uint8_t* out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(out && workspace && H > 0 && W > 0 && M >= 0 && ph > 0 && pw > 0, "stitch_patches: bad arguments");
    CS_CHECK_ARG(M == 0 || (patches && corners), "stitch_patches: NULL patches");
    CS_CHECK_ARG(M <= 65535 && (long long)ph * pw < (1LL << 31), "stitch_patches: too many or too large patches");
    CS_CHECK_ARG(workspace_bytes >= cs_stitch_workspace(H, W), "stitch_patches: workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int32_t* owner = reinterpret_cast<int32_t*>(workspace);
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(stitch_init_kernel, dim3(grid_for(HW)), dim3(256), 0, st, owner, HW);
    CS_LAUNCH_CHECK();
    if (M > 0) {
        hipLaunchKernelGGL(stitch_claim_kernel, dim3(cs_ceil_div((long long)ph * pw, 256), M), dim3(256), 0, st, corners, ph, pw, H, W, owner);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(stitch_gather_kernel, dim3(grid_for(HW)), dim3(256), 0, st, patches, corners, ph, pw, H, W, owner, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stitch_logits(const float* logits, int B, int C, int ph, int pw, int ch, const int32_t* corners, int H, int W,
                                uint8_t* mask, void* stream) {
    CS_CHECK_ARG(mask && H > 0 && W > 0 && B >= 0 && ph > 0 && pw > 0, "stitch_logits: bad arguments");
    CS_CHECK_ARG(C >= 2 && ch >= 0 && ch < C, "stitch_logits: needs at least two channels and 0 <= ch < C");
    CS_CHECK_ARG(B == 0 || (logits && corners), "stitch_logits: NULL logits or corners");
    CS_CHECK_ARG(H < (1 << 29) && W < (1 << 29) && ph <= H && pw <= W, "stitch_logits: the patch must fit the mask, whose sides stay below 2^29");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(corners) & 3) == 0,
                 "stitch_logits: misaligned buffers");
    if (B == 0) return CS_OK;
    const int ng = pw / 4 + 2;                                   // dword units that span a patch row at any alignment
    const long long units = (long long)ph * ng;
    CS_CHECK_ARG(units < (1LL << 30), "stitch_logits: patch too large");
    const int chunks = cs_ceil_div(units, 256);
    hipLaunchKernelGGL(stitch_logits_kernel, dim3(grid_for((long long)B * chunks * 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       logits, corners, B, C, ch, ph, pw, H, W, ng, chunks, mask);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stitch_blend_add(const float* logits, int B, int C, int ph, int pw, int ch, const int32_t* corners, const uint8_t* flips,
                                   const int32_t* taps_r, const int32_t* taps_c, int H, int W, int64_t* num, int32_t* den, void* stream) {
    CS_CHECK_ARG(num && den && taps_r && taps_c && H > 0 && W > 0 && B >= 0 && ph > 0 && pw > 0, "stitch_blend_add: bad arguments");
    CS_CHECK_ARG(C >= 2 && ch >= 0 && ch < C, "stitch_blend_add: needs at least two channels and 0 <= ch < C");
    CS_CHECK_ARG(B == 0 || (logits && corners), "stitch_blend_add: NULL logits or corners");
    CS_CHECK_ARG(H < (1 << 29) && W < (1 << 29) && ph <= H && pw <= W, "stitch_blend_add: the patch must fit the slide, whose sides stay below 2^29");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(corners) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(taps_r) & 3) == 0 && (reinterpret_cast<uintptr_t>(taps_c) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(num) & 15) == 0 && (reinterpret_cast<uintptr_t>(den) & 15) == 0,
                 "stitch_blend_add: misaligned buffers (the accumulators need 16 bytes)");
    CS_CHECK_ARG(B <= 32768, "stitch_blend_add: at most 32768 patches in one call (the sum of their weights stays below 2^31)");
    if (B == 0) return CS_OK;
    const int ng = pw / 4 + 2;                                   // four-pixel units that span a patch row at any alignment
    const long long units = (long long)ph * ng;
    CS_CHECK_ARG(units < (1LL << 30), "stitch_blend_add: patch too large");
    const int chunks = cs_ceil_div(units, 256);
    hipLaunchKernelGGL(stitch_blend_add_kernel, dim3(grid_for((long long)B * chunks * 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       logits, corners, flips, taps_r, taps_c, B, C, ch, ph, pw, H, W, ng, chunks, reinterpret_cast<unsigned long long*>(num),
                       reinterpret_cast<uint32_t*>(den));
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stitch_blend_finish(const int64_t* num, const int32_t* den, int H, int W, uint8_t* mask, void* stream) {
    CS_CHECK_ARG(num && den && mask && H > 0 && W > 0, "stitch_blend_finish: bad arguments");
    CS_CHECK_ARG(H < (1 << 29) && W < (1 << 29), "stitch_blend_finish: the slide's sides stay below 2^29");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(num) & 7) == 0 && (reinterpret_cast<uintptr_t>(den) & 3) == 0, "stitch_blend_finish: misaligned buffers");
    const long long n = (long long)H * W;
    const bool vec = (reinterpret_cast<uintptr_t>(num) & 15) == 0 && (reinterpret_cast<uintptr_t>(den) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    hipLaunchKernelGGL(stitch_blend_finish_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(num), reinterpret_cast<const uint32_t*>(den), n, vec ? n >> 2 : 0LL, mask);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_detect_grid_size(int H, int W, int interval, int window) {
    if (H <= 0 || W <= 0 || interval <= 0 || window <= 0 || window > H || window > W) return -1;
    int a, b;
    const long long g = (long long)axis_count(H, interval, window, &a) * axis_count(W, interval, window, &b);
    return g < (1LL << 31) ? (int)g : -1;
}

extern "C" int cs_detect_meanshift(const uint8_t* blurred, int N, int H, int W, int interval, int window, double thr255, int max_iter,
                                   int32_t* pts, int32_t* n_pts, void* stream) {
    CS_CHECK_ARG(blurred && pts && n_pts && N > 0 && max_iter >= 0, "detect_meanshift: bad arguments");
    CS_CHECK_ARG(window > 0 && window <= kMaxWindow, "detect_meanshift: window size must be in [1, 128]");
    const int G = cs_detect_grid_size(H, W, interval, window);
    CS_CHECK_ARG(G > 0, "detect_meanshift: the window does not fit the map, or the interval is not positive");
    CS_CHECK_ARG((long long)N * G < (1LL << 31), "detect_meanshift: too many windows in one call");
    Grid g;
    g.nr = axis_count(H, interval, window, &g.n0r);
    g.nc = axis_count(W, interval, window, &g.n0c);
    g.interval = interval; g.window = window; g.H = H; g.W = W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(seed_kernel, dim3(N), dim3(1024), 0, st, blurred, g, thr255, pts, n_pts);
    CS_LAUNCH_CHECK();
    const long long HW = (long long)H * W;
    if (HW <= kMsLdsBytes) {
        const size_t lds = (size_t)((HW + 15) & ~15LL);
        if (!cs_allow_dynamic_lds_(reinterpret_cast<const void*>(meanshift_lds_kernel), lds, kMsLdsBytes)) return CS_ERR_LAUNCH;
        hipLaunchKernelGGL(meanshift_lds_kernel, dim3(N), dim3(1024), lds, st, blurred, H, W, G, window, max_iter,
                           pts, n_pts);
    } else {
        hipLaunchKernelGGL(meanshift_global_kernel, dim3(cs_ceil_div((long long)N * G, 4)), dim3(256), 0, st, blurred, N, H, W, G, window,
                           max_iter, pts, n_pts);
    }
    CS_LAUNCH_CHECK();
    return CS_OK;
}

// workspace: lab, cid, wgt (int32 N cap each), cent (int32 2 N cap), key (fp32 N cap), order (int64 N cap), sums (u64 3 N cap),
// n_clu (int32 N), state (int32 2)
extern "C" size_t cs_detect_cluster_workspace(int N, int cap) {
    const size_t t = (size_t)N * cap;
    return cs_align16(t * 4) * 3 + cs_align16(t * 8) + cs_align16(t * 4) + cs_align16(t * 8) + cs_align16(t * 24) + cs_align16((size_t)N * 4) + 16;
}

extern "C" int cs_detect_cluster(const int32_t* pts, const int32_t* n_pts, int N, int cap, double eps, const uint8_t* blurred, int H, int W,
                                 int force_global, int64_t* out_pts, int32_t* out_w, int64_t* out_off, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    CS_CHECK_ARG(pts && n_pts && blurred && out_pts && out_w && out_off && workspace, "detect_cluster: NULL argument");
    CS_CHECK_ARG(N > 0 && N <= 65535 && cap > 0 && H > 0 && W > 0 && (long long)N * cap < (1LL << 31), "detect_cluster: bad sizes");
    CS_CHECK_ARG(eps >= 0.0, "detect_cluster: eps must be non-negative");
    CS_CHECK_ARG(cap <= 65535 * 256, "detect_cluster: too many points per image");
    CS_CHECK_ARG(workspace_bytes >= cs_detect_cluster_workspace(N, cap), "detect_cluster: workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t t = (size_t)N * cap;
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    int32_t* lab = reinterpret_cast<int32_t*>(w);            w += cs_align16(t * 4);
    int32_t* cid = reinterpret_cast<int32_t*>(w);            w += cs_align16(t * 4);
    int32_t* wgt = reinterpret_cast<int32_t*>(w);            w += cs_align16(t * 4);
    int32_t* cent = reinterpret_cast<int32_t*>(w);           w += cs_align16(t * 8);
    float* key = reinterpret_cast<float*>(w);                w += cs_align16(t * 4);
    int64_t* order = reinterpret_cast<int64_t*>(w);          w += cs_align16(t * 8);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(w); w += cs_align16(t * 24);
    int32_t* n_clu = reinterpret_cast<int32_t*>(w);          w += cs_align16((size_t)N * 4);
    int32_t* state = reinterpret_cast<int32_t*>(w);
    const double eps2 = eps * eps;
    if (cap <= kLdsPts && !force_global) {
        hipLaunchKernelGGL(cluster_lds_kernel, dim3(N), dim3(1024), 0, st, pts, n_pts, cap, eps2, lab);
        CS_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(cluster_init_kernel, dim3(grid_for((long long)t)), dim3(256), 0, st, n_pts, N, cap, lab, state);
        CS_LAUNCH_CHECK();
        const int tiles = cs_ceil_div(cap, 256);
        // rounds are enqueued eight at a time; once a round hooks nothing, the launches still queued return at once.  The host
        // reads the done flag between groups (a handful of components need more than eight rounds).
        for (int group = 0;; ++group) {
            for (int r = 0; r < 8; ++r) {
                hipLaunchKernelGGL(cluster_hook_kernel, dim3(tiles, tiles, N), dim3(256), 0, st, pts, n_pts, cap, eps2, lab, state);
                CS_LAUNCH_CHECK();
                hipLaunchKernelGGL(cluster_jump_kernel, dim3(grid_for((long long)t)), dim3(256), 0, st, n_pts, N, cap, lab, state);
                CS_LAUNCH_CHECK();
                hipLaunchKernelGGL(cluster_round_end_kernel, dim3(1), dim3(1), 0, st, state);
                CS_LAUNCH_CHECK();
            }
            int32_t done = 0;
            if (hipMemcpyAsync(&done, state + 1, sizeof(done), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) {
                cs_set_error_("detect_cluster: cannot read the convergence flag");
                return CS_ERR_LAUNCH;
            }
            if (done) break;
            if (group >= 4096) {
                cs_set_error_("detect_cluster: clustering did not converge");
                return CS_ERR_LAUNCH;
            }
        }
    }
    hipLaunchKernelGGL(cluster_ids_kernel, dim3(N), dim3(1024), 0, st, n_pts, cap, lab, cid, n_clu, sums);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_accum_kernel, dim3(grid_for((long long)t)), dim3(256), 0, st, pts, n_pts, N, cap, lab, cid, sums);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_offsets_kernel, dim3(1), dim3(256), 0, st, n_clu, N, out_off);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_centroid_kernel, dim3(grid_for((long long)t)), dim3(256), 0, st, n_clu, N, cap, sums, out_off, blurred, H, W,
                       key, cent, wgt);
    CS_LAUNCH_CHECK();
    const int rc = cs_segmented_order(key, out_off, N, cap, (long long)t, order, stream);
    if (rc != CS_OK) return rc;
    hipLaunchKernelGGL(cluster_emit_kernel, dim3(grid_for((long long)t)), dim3(256), 0, st, n_clu, N, cap, out_off, order, cent, wgt, out_pts,
                       out_w);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
