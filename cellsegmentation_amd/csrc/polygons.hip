// Polygons to pixels (polygons.py is the public API): scan conversion of many small shapes and a few huge ones into an int32 label
// image or a uint8 mask, in exact integer arithmetic.  The rule is the one of cs_polygons_rasterize in include/cellseg_hip.h: the
// centre of a pixel decides, the ray runs towards smaller columns, no float is involved anywhere.
//
// One launch, a workgroup of 256 per ITEM = (shape, first row, rows); without an item table an item is a whole shape and the
// workgroup reduces the shape's row range from its vertices first.  The shape's edges go through LDS kChunk at a time as
// (ya, xa, yb, xb) in units of 1 / (2 S) pixel.  The four waves take four consecutive rows.  For its row a wave tests 64 staged
// edges per step against the centre line Y; the test is per lane, the ballot of it is wave-uniform.  An edge that spans the line
// is reduced, by a bisection over 64-bit integer products, to the first column jc whose centre it counts for: the pixel test
// d > 0 ? cross <= 0 : cross >= 0 is X |d| >= K with K = +-((xb - xa)(Y - ya) + xa d), and X = (2 j + 1) S rises with j.  The
// events (jc, +-1), jc cut to [0, W], are compacted by ballot and prefix into the wave's list; the list survives the chunks of a
// shape, so a shape of any number of edges is summed before the rule (even-odd or non-zero) is applied.  Then the wave walks the
// 64-column segments between the smallest and the largest jc, a pixel per lane: the winding number of pixel j is the sum of the
// signs of the events with jc <= j, and from the largest jc on it is 0, because the spanning edges of closed rings cancel.  Per
// segment the list is read 64 events at a time, one per lane: the events at or before the segment's first column count for all 64
// pixels alike (two ballots), and only those that begin inside the segment are held against each pixel, by LDS broadcast.
// A row with more than kList events is evaluated straight from the rule instead: every edge of the shape, read from global
// memory with wave-uniform addresses, against every pixel of the row (E W / 64 steps for that row).
// A shape with at most kChunk edges is staged once for all its rows, a larger one once per four rows.
// Labels go out by raise_to (a relaxed load, then an integer maximum at device scope): the highest label wins whatever the order
// of arrival.  The mask goes out as plain byte stores of 1.  The grid depends on the number of items alone and is capped.
#include "cs_common.h"
#include "cs_block.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 1024;                       // edges staged at a time: 16 KiB of LDS
constexpr int kList = 256;                         // events a wave keeps for its row: 1 KiB of LDS per wave
constexpr int kMaxBlocks = 1 << 16;
constexpr int kGlobal = __HIP_MEMORY_SCOPE_AGENT;

struct PolyArgs {
    const int32_t* vertices;                       // [V][2] = (row, col) in units of 1 / S pixel
    const int32_t* ring_start;                     // [R]
    const int32_t* ring_count;                     // [R]
    const int32_t* shape_rings;                    // [S + 1]
    const int32_t* image_shapes;                   // [N + 1]
    const int32_t* items;                          // [I][3] or NULL
    long long V, I;
    int R, S, N, H, W, sub;
};

__device__ __forceinline__ void raise_to(int32_t* p, int x) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, kGlobal) < x) __hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, kGlobal);
}

// ring r as (first vertex row, vertices); a ring that does not lie inside the vertex table has none
__device__ __forceinline__ void ring_of(const PolyArgs& a, int r, long long& start, int& count) {
    start = a.ring_start[r];
    count = a.ring_count[r];
    if (count <= 0 || start < 0 || start + count > a.V) count = 0;
}

// edge k of a ring: vertex k -> vertex k + 1, the last one back to the first; y = 2 row, x = 2 col
__device__ __forceinline__ int4 edge_of(const PolyArgs& a, long long start, int count, int k) {
    const int2 p = reinterpret_cast<const int2*>(a.vertices)[start + k];
    const int2 q = reinterpret_cast<const int2*>(a.vertices)[start + (k + 1 == count ? 0 : k + 1)];
    return make_int4(2 * p.x, 2 * p.y, 2 * q.x, 2 * q.y);
}

// the first row whose centre line Y = (2 i + 1) S is not below y: ceil((y - S) / (2 S)), an arithmetic shift floors
__device__ __forceinline__ int first_row_at(int y, int sub) { return (y + (1 << sub) - 1) >> (sub + 1); }

// the smallest j in [0, W] with (2 j + 1) S D >= K (W: none in the image); (2 j + 1) S < 2^30 and D <= 2^30
__device__ __forceinline__ int first_column(long long K, int D, int sub, int W) {
    int lo = 0, hi = W;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)((2 * mid + 1) << sub) * D >= K) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ bool taken(int wind, int rule) { return rule == CS_POLYGON_NONZERO ? wind != 0 : (wind & 1) != 0; }

template <bool MASK>
__device__ __forceinline__ void put(void* out, long long at, int label) {
    if (MASK) reinterpret_cast<uint8_t*>(out)[at] = 1;
    else raise_to(reinterpret_cast<int32_t*>(out) + at, label);
}

// grid (min(items, kMaxBlocks))
template <bool MASK>
__global__ __launch_bounds__(kThreads) void polygons_rasterize_kernel(PolyArgs a, int rule, void* __restrict__ out) {
    __shared__ int4 s_edge[kChunk];
    __shared__ uint32_t s_list[kWaves][kList];
    __shared__ int s_slot[kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long n_items = a.items ? a.I : (long long)a.S;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {         // uniform: every thread reaches the barriers
        const int s = a.items ? a.items[3 * it] : (int)it;
        if (s < 0 || s >= a.S) continue;
        const int ring0 = max(a.shape_rings[s], 0), ring1 = min(a.shape_rings[s + 1], a.R);
        // the image of the shape: the last n with image_shapes[n] <= s
        int n = 0;
        for (int hi = a.N - 1; n < hi;) {
            const int mid = (n + hi + 1) >> 1;
            if (a.image_shapes[mid] <= s) n = mid;
            else hi = mid - 1;
        }
        const int label = s - a.image_shapes[n] + 1;
        if (label < 1 || s >= a.image_shapes[n + 1]) continue;

        // the edges of the shape and, without an item table, its rows
        long long total = 0;
        int r0, r1;
        if (a.items) {
            for (int r = ring0; r < ring1; ++r) {
                long long start;
                int count;
                ring_of(a, r, start, count);
                total += count;
            }
            r0 = a.items[3 * it + 1];
            r1 = r0 + max(a.items[3 * it + 2], 0);
        } else {
            int ylo = INT32_MAX, yhi = INT32_MIN;
            for (int r = ring0; r < ring1; ++r) {
                long long start;
                int count;
                ring_of(a, r, start, count);
                total += count;
                for (int k = threadIdx.x; k < count; k += kThreads) {
                    const int y = 2 * a.vertices[2 * (start + k)];
                    ylo = min(ylo, y);
                    yhi = max(yhi, y);
                }
            }
            ylo = block_reduce<kThreads, int>(ylo, [](int x, int y) { return min(x, y); }, s_slot);
            yhi = block_reduce<kThreads, int>(yhi, [](int x, int y) { return max(x, y); }, s_slot);
            if (ylo > yhi) continue;                                         // no vertex at all
            r0 = first_row_at(ylo, a.sub);                                   // a spanned centre line has ylo <= Y < yhi
            r1 = first_row_at(yhi, a.sub);
        }
        r0 = max(r0, 0);
        r1 = min(r1, a.H);
        if (total == 0 || r0 >= r1) continue;
        const bool once = total <= kChunk;
        const long long plane = (long long)n * a.H;

        for (int g0 = r0; g0 < r1; g0 += kWaves) {
            const int row = g0 + wv;
            const bool live = row < r1;
            const int Y = (2 * row + 1) << a.sub;
            int cnt = 0, jlo = INT32_MAX, jhi = INT32_MIN;                   // cnt is wave-uniform
            int ring = ring0;
            long long base = 0;                                              // the shape's edges before `ring`
            for (long long c0 = 0; c0 < total; c0 += kChunk) {
                const int n_e = (int)min((long long)kChunk, total - c0);
                if (!once || g0 == r0) {
                    __syncthreads();                                         // the waves are done with the chunk before
                    while (ring < ring1) {
                        long long start;
                        int count;
                        ring_of(a, ring, start, count);
                        const long long lo = max(base, c0), hi = min(base + count, c0 + kChunk);
                        for (long long e = lo + threadIdx.x; e < hi; e += kThreads) s_edge[e - c0] = edge_of(a, start, count, (int)(e - base));
                        if (base + count > c0 + kChunk) break;               // the ring goes on in the next chunk
                        base += count;
                        ++ring;
                    }
                    __syncthreads();
                }
                if (!live) continue;
                for (int e0 = 0; e0 < n_e; e0 += 64) {
                    const int e = e0 + lane;
                    const int4 ed = s_edge[min(e, n_e - 1)];
                    const int ya = ed.x, xa = ed.y, yb = ed.z, xb = ed.w;
                    bool keep = e < n_e && (ya <= Y) != (yb <= Y);
                    if (!__any(keep)) continue;
                    int jc = 0;
                    const int d = yb - ya;
                    if (keep) {
                        const long long K = (long long)(xb - xa) * (Y - ya) + (long long)xa * d;
                        jc = first_column(d > 0 ? K : -K, abs(d), a.sub, a.W);   // W: it counts for no pixel of the image
                    }
                    const unsigned long long bal = __ballot(keep);
                    const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull));
                    if (keep) {
                        if (pos < kList) s_list[wv][pos] = ((uint32_t)jc << 1) | (d > 0 ? 1u : 0u);
                        jlo = min(jlo, jc);
                        jhi = max(jhi, jc);
                    }
                    cnt += __popcll(bal);
                }
            }
            if (!live || cnt == 0) continue;                                 // no barrier below: the waves part here
            const long long line = (plane + row) * a.W;
            if (cnt <= kList) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    jlo = min(jlo, __shfl_xor(jlo, off));
                    jhi = max(jhi, __shfl_xor(jhi, off));
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the list was written by other lanes of this wave
                for (int j0 = jlo & ~63; j0 < jhi; j0 += 64) {
                    const int j = j0 + lane;
                    int wind = 0;
                    for (int k0 = 0; k0 < cnt; k0 += 64) {                   // 64 events per step, one per lane
                        const int k = k0 + lane;
                        const uint32_t ev = s_list[wv][min(k, cnt - 1)];
                        const int jc = (int)(ev >> 1);
                        const bool up = (ev & 1u) != 0, before = k < cnt && jc <= j0;
                        wind += __popcll(__ballot(before && up)) - __popcll(__ballot(before && !up));     // the same for all 64 pixels
                        unsigned long long in = __ballot(k < cnt && jc > j0 && jc <= j0 + 63);
                        while (in) {                                         // wave-uniform: the events that begin inside the segment
                            const uint32_t e = s_list[wv][k0 + __builtin_ctzll(in)];
                            in &= in - 1;
                            if ((int)(e >> 1) <= j) wind += (e & 1u) ? 1 : -1;
                        }
                    }
                    if (j >= jlo && j < jhi && taken(wind, rule)) put<MASK>(out, line + j, label);
                }
            } else {
                for (int j0 = 0; j0 < a.W; j0 += 64) {
                    const int j = j0 + lane;
                    const int X = (2 * min(j, a.W - 1) + 1) << a.sub;
                    int wind = 0;
                    for (int r = ring0; r < ring1; ++r) {
                        long long start;
                        int count;
                        ring_of(a, r, start, count);
                        for (int k = 0; k < count; ++k) {
                            const int4 ed = edge_of(a, start, count, k);
                            const int ya = ed.x, xa = ed.y, yb = ed.z, xb = ed.w, d = yb - ya;
                            if ((ya <= Y) == (yb <= Y)) continue;            // wave-uniform
                            const long long cross = (long long)(xb - xa) * (Y - ya) - (long long)(X - xa) * d;
                            if (d > 0 ? cross <= 0 : cross >= 0) wind += d > 0 ? 1 : -1;
                        }
                    }
                    if (j < a.W && taken(wind, rule)) put<MASK>(out, line + j, label);
                }
            }
        }
    }
}

}  // namespace

static inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

extern "C" int cs_polygons_rasterize(const int32_t* vertices, long long V, const int32_t* ring_start, const int32_t* ring_count, int R,
                                     const int32_t* shape_rings, int S, const int32_t* image_shapes, const int32_t* items, long long I, int N,
                                     int H, int W, int sub, int rule, int mode, void* out, void* stream) {
    CS_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1LL << 31),
                 "polygons_rasterize: need 0 < N <= 65535 images of 0 < H W < 2^31 pixels");
    CS_CHECK_ARG(sub >= 0 && sub <= 8 && ((long long)(H > W ? H : W) << (sub + 1)) < (1LL << 30),
                 "polygons_rasterize: need 0 <= sub <= 8 and max(H, W) << (sub + 1) < 2^30");
    CS_CHECK_ARG(rule == CS_POLYGON_EVENODD || rule == CS_POLYGON_NONZERO, "polygons_rasterize: unknown rule");
    CS_CHECK_ARG(mode == CS_POLYGON_LABELS || mode == CS_POLYGON_MASK, "polygons_rasterize: unknown mode");
    CS_CHECK_ARG(V >= 0 && V < (1LL << 31) && R >= 0 && S >= 0 && I >= 0 && I < (1LL << 31), "polygons_rasterize: need 0 <= V, R, S, I < 2^31");
    CS_CHECK_ARG(out && shape_rings && image_shapes && ((vertices && ring_start && ring_count) || R == 0 || V == 0),
                 "polygons_rasterize: NULL argument");
    CS_CHECK_ARG(aligned(vertices, 8) && aligned(ring_start, 4) && aligned(ring_count, 4) && aligned(shape_rings, 4) && aligned(image_shapes, 4) &&
                     aligned(items, 4) && (mode == CS_POLYGON_MASK || aligned(out, 4)),
                 "polygons_rasterize: misaligned argument");
    const long long n_items = items ? I : (long long)S;
    if (n_items == 0 || R == 0 || V == 0) return CS_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PolyArgs a{vertices, ring_start, ring_count, shape_rings, image_shapes, items, V, I, R, S, N, H, W, sub};
    const dim3 grid((unsigned)(n_items < kMaxBlocks ? n_items : kMaxBlocks));
    if (mode == CS_POLYGON_MASK) hipLaunchKernelGGL(polygons_rasterize_kernel<true>, grid, dim3(kThreads), 0, st, a, rule, out);
    else hipLaunchKernelGGL(polygons_rasterize_kernel<false>, grid, dim3(kThreads), 0, st, a, rule, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
