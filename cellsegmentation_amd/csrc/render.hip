// Annotated images (render.py is the public API): what the reference draws on the host with numpy and OpenCV -- the half-white mask
// overlay, the colour-mapped heat map, object outlines and the dots of the detected cells -- drawn where the slide, its mask and its
// points already are.  Two kernels, all integer:
//   compose  one pass over the pixels of uint8 [N][H][W][3]: an optional fill (mask overlay, or heat map through a 256-entry colour
//            table), then an optional outline from a label image by the edge rule of regions.hip's edge_kernel, evaluated here so
//            that no edge map is ever stored.  The image is read once and written once.  The batch is one flat run of N H W pixels
//            (only the outline rule needs rows and columns).  The unit of work is 4 pixels = 12 bytes = three dwords: the fills are
//            byte-parallel dword arithmetic on those three words, the per-pixel operands (mask flag, table colour, outline colour)
//            being spread over them by pack4.  The pixels are walked by cs_pixels.h, a run of 16 being four units; the single pixels
//            on either side go through the same arithmetic, and no alignment is asked of anything.  The outline of a run reads its
//            own 16 labels and the 16 above and below once each (the neighbours left and right are its own), with one division
//            per run; a first version that asked label by label -- a division and four loads per labelled pixel, in divergent
//            code -- ran at 18 times the copy.  The colour table and the palette sit in LDS as packed words.  The grid is capped and
//            strides; every pixel depends on its own inputs alone.
//   points   a scatter: one wave per row of the points buffer (the ragged point set of cs_points.h: the rows its windows keep, or
//            with `tail` the rows of a window that its limit does not keep), its lanes over the box of the disc or ring, byte
//            stores.  Every store of a launch carries the same colour, so marks that overlap do not depend on the order of arrival.
#include <limits.h>
#include "cs_common.h"
#include "cs_pixels.h"
#include "cs_points.h"

namespace {

constexpr int kThreads = 256;                      // also the rows of the colour table: thread v stages entry v
constexpr int kMaxRadius = 64;

struct ComposeArgs {
    const uint8_t* img;                            // [T][3]; may be `out`
    uint8_t* out;
    const void* fill;                              // uint8 [T] or fp32 [T], by the kernel's FILL
    const uint8_t* cmap;                           // [256][3]
    const int32_t* lab;                            // [T] or NULL
    const uint8_t* pal;                            // [pal_rows][3] or NULL
    long long T;                                   // N H W < 2^31
    int H, W, invert, pal_rows;
    float thr;
    uint32_t outline;                              // r | g << 8 | b << 16
};

__device__ __forceinline__ uint32_t rgb_at(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }

// four 24-bit values, one per pixel, laid over the three dwords that hold those four pixels
__device__ __forceinline__ void pack4(const uint32_t* k, uint32_t* K) {
    K[0] = k[0] | k[1] << 24;
    K[1] = k[1] >> 8 | k[2] << 16;
    K[2] = k[2] >> 16 | k[3] << 8;
}

// the heat level of a probability: p > thr ? (uint8)(255.0f * p) : 0
__device__ __forceinline__ uint32_t heat_level(float p, float thr) { return p > thr ? (uint32_t)(int)(255.0f * p) & 255u : 0u; }

// the fill of 4 pixels in the dwords w[0..2]; f[i]: the mask byte or the heat level of pixel i
template <int FILL>
__device__ __forceinline__ void shade4(uint32_t* w, const uint32_t* f, const ComposeArgs& a, const uint32_t* s_cmap) {
    if (FILL == CS_RENDER_FILL_NONE) return;
    uint32_t k[4], K[3];
    if (FILL == CS_RENDER_FILL_MASK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = f[i] ? 0xffffffu : 0u;
        pack4(k, K);
#pragma unroll
        for (int d = 0; d < 3; ++d) {              // per byte: c >> 1, and (c + 255) >> 1 = (c >> 1) + (c & 1) + 127
            const uint32_t half = (w[d] >> 1) & 0x7f7f7f7fu;
            const uint32_t on = half + (w[d] & 0x01010101u) + 0x7f7f7f7fu;
            w[d] = (on & K[d]) | (half & ~K[d]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = s_cmap[a.invert ? 255u - f[i] : f[i]];
        pack4(k, K);
#pragma unroll
        for (int d = 0; d < 3; ++d) {              // per byte: floor((c + k) / 2) = (c & k) + ((c ^ k) >> 1), + 1 where the sum is
            const uint32_t x = w[d] ^ K[d];        // odd and the floor is odd: the mean rounded half to even
            const uint32_t fl = (w[d] & K[d]) + ((x >> 1) & 0x7f7f7f7fu);
            w[d] = fl + (x & fl & 0x01010101u);
        }
    }
}

// the id of pixel p if it is an edge pixel of its object, else 0 (edge_kernel of regions.hip)
__device__ __forceinline__ int edge_id(const ComposeArgs& a, uint32_t p) {
    const int l = a.lab[p];
    if (l <= 0) return 0;
    const uint32_t q = p / (uint32_t)a.W;
    const int c = (int)(p - q * (uint32_t)a.W), r = (int)(q % (uint32_t)a.H);
    const int left = c > 0 ? max(a.lab[p - 1], 0) : 0, right = c + 1 < a.W ? max(a.lab[p + 1], 0) : 0;
    const int up = r > 0 ? max(a.lab[p - a.W], 0) : 0, down = r + 1 < a.H ? max(a.lab[p + a.W], 0) : 0;
    return (left != l || right != l || up != l || down != l) ? l : 0;
}

// the outline over the `count` <= 4 pixels from p on, in the dwords w[0..2]
__device__ __forceinline__ void outline4(uint32_t* w, const ComposeArgs& a, uint32_t p, int count, const uint32_t* s_pal) {
    uint32_t e[4], col[4], M[3], C[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = i < count ? edge_id(a, p + i) : 0;
        e[i] = id ? 0xffffffu : 0u;
        col[i] = !id ? 0u : a.pal_rows ? s_pal[(uint32_t)(id - 1) % (uint32_t)a.pal_rows] : a.outline;
    }
    pack4(e, M);
    pack4(col, C);
#pragma unroll
    for (int d = 0; d < 3; ++d) w[d] = C[d] | (w[d] & ~M[d]);
}

// the ids max(label, 0) of the kPixelRun pixels at q; vec: q is 16-byte aligned
__device__ __forceinline__ void ids16(const int32_t* q, bool vec, int (&v)[kPixelRun]) {
    if (vec) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 x = reinterpret_cast<const int4*>(q)[j];
            v[4 * j] = max(x.x, 0), v[4 * j + 1] = max(x.y, 0), v[4 * j + 2] = max(x.z, 0), v[4 * j + 3] = max(x.w, 0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPixelRun; ++i) v[i] = max(q[i], 0);
    }
}

// the outline over the kPixelRun pixels from p on, in the dwords w[0..11]: the rule of edge_id with the run's own labels and the runs
// above and below it loaded once -- as vectors where they are aligned (vec_c: this run; vec_ud: W is a multiple of 4 as well) --
// and one division for the run, the row and column stepping from pixel to pixel.  A run may cross rows and images.
__device__ __forceinline__ void outline16(uint32_t* w, const ComposeArgs& a, long long p, bool vec_c, bool vec_ud, const uint32_t* s_pal) {
    int ctr[kPixelRun], up[kPixelRun], dn[kPixelRun];
    ids16(a.lab + p, vec_c, ctr);
    int any = 0;
#pragma unroll
    for (int i = 0; i < kPixelRun; ++i) any |= ctr[i];
    if (!any) return;                              // background only, as most of a slide is: no neighbour is looked at
    if (p >= a.W) {                             // the whole run above lies in the buffer (a first row's is not used)
        ids16(a.lab + p - a.W, vec_ud, up);
    } else {
#pragma unroll
        for (int i = 0; i < kPixelRun; ++i) up[i] = p + i >= a.W ? max(a.lab[p + i - a.W], 0) : 0;
    }
    if (p + a.W + kPixelRun <= a.T) {
        ids16(a.lab + p + a.W, vec_ud, dn);
    } else {
#pragma unroll
        for (int i = 0; i < kPixelRun; ++i) dn[i] = p + i + a.W < a.T ? max(a.lab[p + i + a.W], 0) : 0;
    }
    const uint32_t q = (uint32_t)p / (uint32_t)a.W;
    int c = (int)((uint32_t)p - q * (uint32_t)a.W), r = (int)(q % (uint32_t)a.H);
    const int before = c > 0 ? max(a.lab[p - 1], 0) : 0;
    uint32_t e[kPixelRun], col[kPixelRun];
#pragma unroll
    for (int i = 0; i < kPixelRun; ++i) {
        const int l = ctr[i];
        const int left = c == 0 ? 0 : i ? ctr[i ? i - 1 : 0] : before;
        int right = 0;
        if (c + 1 < a.W) right = i + 1 < kPixelRun ? ctr[i + 1 < kPixelRun ? i + 1 : i] : max(a.lab[p + kPixelRun], 0);      // the same row: inside the buffer
        const int above = r > 0 ? up[i] : 0, below = r + 1 < a.H ? dn[i] : 0;
        const bool edge = l > 0 && (left != l || right != l || above != l || below != l);
        e[i] = edge ? 0xffffffu : 0u;
        col[i] = 0;
        if (edge) col[i] = a.pal_rows ? s_pal[(uint32_t)(l - 1) % (uint32_t)a.pal_rows] : a.outline;
        if (++c == a.W) {
            c = 0;
            if (++r == a.H) r = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t M[3], C[3];
        pack4(e + 4 * j, M);
        pack4(col + 4 * j, C);
#pragma unroll
        for (int d = 0; d < 3; ++d) w[3 * j + d] = C[d] | (w[3 * j + d] & ~M[d]);
    }
}

// the fill operand of pixel p alone
template <int FILL>
__device__ __forceinline__ uint32_t fill_at(const ComposeArgs& a, long long p) {
    if (FILL == CS_RENDER_FILL_NONE) return 0;
    if (FILL == CS_RENDER_FILL_HEAT_F32) return heat_level(static_cast<const float*>(a.fill)[p], a.thr);
    return static_cast<const uint8_t*>(a.fill)[p];
}

// the fill operands of the kPixelRun pixels from p on; width: the access_width of the map's first run
template <int FILL>
__device__ __forceinline__ void fill16(const ComposeArgs& a, long long p, int width, uint32_t (&f)[kPixelRun]) {
    if (FILL == CS_RENDER_FILL_NONE) return;
    if (FILL == CS_RENDER_FILL_HEAT_F32) {
        const float* q = static_cast<const float*>(a.fill) + p;
        if (width == 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = reinterpret_cast<const float4*>(q)[j];
                f[4 * j] = heat_level(v.x, a.thr), f[4 * j + 1] = heat_level(v.y, a.thr);
                f[4 * j + 2] = heat_level(v.z, a.thr), f[4 * j + 3] = heat_level(v.w, a.thr);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPixelRun; ++i) f[i] = heat_level(q[i], a.thr);
        }
        return;
    }
    uint32_t m[4];
    load_bytes16(static_cast<const uint8_t*>(a.fill) + p, width, m);
#pragma unroll
    for (int i = 0; i < kPixelRun; ++i) f[i] = byte_of(m, i);
}

// pixel p alone, through the arithmetic of a unit whose other three pixels are not stored
template <int FILL>
__device__ __forceinline__ void compose_one(const ComposeArgs& a, long long p, const uint32_t* s_cmap, const uint32_t* s_pal) {
    uint32_t w[3] = {rgb_at(a.img + 3 * p), 0, 0};
    const uint32_t f[4] = {fill_at<FILL>(a, p), 0, 0, 0};
    shade4<FILL>(w, f, a, s_cmap);
    if (a.lab) outline4(w, a, (uint32_t)p, 1, s_pal);
    uint8_t* q = a.out + 3 * p;
    q[0] = (uint8_t)w[0], q[1] = (uint8_t)(w[0] >> 8), q[2] = (uint8_t)(w[0] >> 16);
}

// grid (capped): the batch as one span of T pixels
template <int FILL>
__global__ __launch_bounds__(kThreads) void render_compose_kernel(const ComposeArgs a) {
    __shared__ uint32_t s_cmap[256], s_pal[256];
    const int tid = threadIdx.x;
    if (FILL == CS_RENDER_FILL_HEAT_U8 || FILL == CS_RENDER_FILL_HEAT_F32) s_cmap[tid] = rgb_at(a.cmap + 3 * tid);
    if (tid < a.pal_rows) s_pal[tid] = rgb_at(a.pal + 3 * tid);
    __syncthreads();
    const PixelSpan s = pixel_span(a.img, a.T);
    const int out_width = access_width(a.out + 3 * s.head);
    const bool lab_vec = a.lab && access_width(a.lab + s.head) == 16;
    const int fill_width = FILL == CS_RENDER_FILL_NONE           ? 1
                           : FILL == CS_RENDER_FILL_HEAT_F32     ? access_width(static_cast<const float*>(a.fill) + s.head)
                                                                 : access_width(static_cast<const uint8_t*>(a.fill) + s.head);
    for_pixels<kThreads>(
        s,
        [&](long long g, uint32_t(&w)[12]) {
            const long long p = s.head + kPixelRun * g;
            uint32_t f[kPixelRun];
            fill16<FILL>(a, p, fill_width, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) shade4<FILL>(w + 3 * j, f + 4 * j, a, s_cmap);
            if (a.lab) outline16(w, a, p, lab_vec, lab_vec && (a.W & 3) == 0, s_pal);
            store_words(a.out + 3 * p, out_width, w);
        },
        [&](long long p) { compose_one<FILL>(a, p, s_cmap, s_pal); });
}

struct PointArgs {
    uint8_t* canvas;                               // [N][H][W][3]
    PointSet p;
    int N, H, W, radius, thickness, tail;
    uint32_t rgb;
};

// grid (ceil(P / 4)): wave w of a workgroup takes row 4 blockIdx.x + w of the points buffer
__global__ __launch_bounds__(kThreads) void render_points_kernel(const PointArgs a) {
    const long long i = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int n = i < a.p.P ? point_image(a.p, a.N, i) : -1;
    if (n < 0) return;
    const PointWindow w = point_window(a.p, n);
    if (!w.ok || (i - w.o0 < w.kept) == (a.tail != 0)) return;
    const long long pr = a.p.pts[2 * i + a.p.xy], pc = a.p.pts[2 * i + 1 - a.p.xy];
    const int t = a.thickness, R = t < 0 ? a.radius : a.radius + (t + 1) / 2;      // the box holds every pixel of the mark
    if (pr < -R || pr >= (long long)a.H + R || pc < -R || pc >= (long long)a.W + R) return;
    const int side = 2 * R + 1, r2 = a.radius * a.radius;
    const int in2 = (2 * a.radius - t) * (2 * a.radius - t), out2 = (2 * a.radius + t) * (2 * a.radius + t);
    for (int j = lane; j < side * side; j += 64) {
        const int dr = j / side - R, dc = j % side - R, d2 = dr * dr + dc * dc;
        const bool on = t < 0 ? d2 <= r2 : (in2 <= 4 * d2 && 4 * d2 <= out2);
        const int r = (int)pr + dr, c = (int)pc + dc;
        if (!on || r < 0 || r >= a.H || c < 0 || c >= a.W) continue;
        uint8_t* q = a.canvas + (((long long)n * a.H + r) * a.W + c) * 3;
        q[0] = (uint8_t)a.rgb, q[1] = (uint8_t)(a.rgb >> 8), q[2] = (uint8_t)(a.rgb >> 16);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <int FILL>
void launch_compose(const ComposeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(render_compose_kernel<FILL>, pixel_grid(1, a.T, kThreads), dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" int cs_render_compose(const uint8_t* images_hwc, int N, int H, int W, int fill, const void* fill_map, float threshold, int invert,
                                 const uint8_t* colormap, const int32_t* labels, int outline_rgb, const uint8_t* palette, int palette_rows,
                                 uint8_t* out, void* stream) {
    CS_CHECK_ARG(pixel_batch_ok(N, H, W), "render_compose: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(fill >= CS_RENDER_FILL_NONE && fill <= CS_RENDER_FILL_HEAT_F32, "render_compose: unknown fill");
    CS_CHECK_ARG(images_hwc && out, "render_compose: NULL argument");
    CS_CHECK_ARG((fill == CS_RENDER_FILL_NONE) == (fill_map == nullptr), "render_compose: a fill needs its map, no fill takes none");
    const bool heat = fill == CS_RENDER_FILL_HEAT_U8 || fill == CS_RENDER_FILL_HEAT_F32;
    CS_CHECK_ARG(!heat || colormap, "render_compose: a heat fill needs the colour table");
    CS_CHECK_ARG(palette_rows >= 0 && palette_rows <= 256 && (palette_rows > 0) == (palette != nullptr),
                 "render_compose: need a palette of 1 to 256 rows, or none and 0 rows");
    CS_CHECK_ARG(labels || !palette, "render_compose: a palette needs the labels");
    CS_CHECK_ARG(outline_rgb >= 0 && outline_rgb < (1 << 24), "render_compose: outline_rgb is r | g << 8 | b << 16");
    CS_CHECK_ARG(aligned(labels, 4) && (fill != CS_RENDER_FILL_HEAT_F32 || aligned(fill_map, 4)), "render_compose: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const ComposeArgs a{images_hwc, out, fill_map, colormap, labels, palette, (long long)N * H * W, H, W, invert != 0, palette_rows,
                        threshold, (uint32_t)outline_rgb};
    if (fill == CS_RENDER_FILL_MASK) launch_compose<CS_RENDER_FILL_MASK>(a, st);
    else if (fill == CS_RENDER_FILL_HEAT_U8) launch_compose<CS_RENDER_FILL_HEAT_U8>(a, st);
    else if (fill == CS_RENDER_FILL_HEAT_F32) launch_compose<CS_RENDER_FILL_HEAT_F32>(a, st);
    else launch_compose<CS_RENDER_FILL_NONE>(a, st);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_render_points(uint8_t* canvas_hwc, int N, int H, int W, const int64_t* pts, const int64_t* off, const int32_t* limit,
                                long long P, int radius, int thickness, int rgb, int flags, void* stream) {
    CS_CHECK_ARG(pixel_batch_ok(N, H, W), "render_points: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(P >= 0 && P < (1LL << 31), "render_points: need 0 <= P < 2^31 rows");
    CS_CHECK_ARG(radius >= 0 && radius <= kMaxRadius, "render_points: need 0 <= radius <= 64");
    CS_CHECK_ARG(thickness < 0 || (thickness >= 1 && thickness <= 2 * radius), "render_points: need thickness < 0 or 1 <= thickness <= 2 radius");
    CS_CHECK_ARG(rgb >= 0 && rgb < (1 << 24), "render_points: rgb is r | g << 8 | b << 16");
    CS_CHECK_ARG(flags >= 0 && flags <= (CS_RENDER_POINTS_XY | CS_RENDER_POINTS_TAIL), "render_points: unknown flags");
    CS_CHECK_ARG(limit || !(flags & CS_RENDER_POINTS_TAIL), "render_points: the tail needs the limits");
    CS_CHECK_ARG(canvas_hwc && off && (pts || P == 0), "render_points: NULL argument");
    CS_CHECK_ARG(aligned(pts, 8) && aligned(off, 8) && aligned(limit, 4), "render_points: misaligned argument");
    if (P == 0) return CS_OK;
    const PointArgs a{canvas_hwc, {pts, off, limit, P, flags & CS_RENDER_POINTS_XY ? 1 : 0}, N, H, W, radius, thickness,
                      flags & CS_RENDER_POINTS_TAIL ? 1 : 0, (uint32_t)rgb};
    const unsigned blocks = (unsigned)((P + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(render_points_kernel, dim3(blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
