// Small-region clean-up of binary masks (utils/image_processing.py:14-17 remove_small_regions = skimage remove_small_objects, then
// remove_small_holes; both are scipy.ndimage.label + an area filter):
//   label     every pixel gets the lowest row-major index of its component of EQUAL-VALUED neighbours (4- or 8-neighbourhood), so
//             one pass labels the foreground components and the background components at once:
//               tiles   a 64 x 64 tile per workgroup, union-find in LDS, flattened; the tile-local pixel count of every tile-local
//                       root is left in the area array at the root's slot (0 elsewhere)
//               borders one thread per pixel of a tile's first row / first column unites across the tile edge (and, with
//                       connectivity 2, across the corner) with global atomicMin hooks
//               flatten every pixel takes its root; a tile-local root that is no longer a root adds its count to the root's slot
//   filter    out = the other value where the pixel has the wanted value and area[root] < threshold (strict), else the input
//   number    scipy's numbering of the foreground: 1 + the number of foreground roots with a lower index in the same image
//   measure   one table row per numbered component (area, bounding box, row / column / intensity sums, intensity maximum): integer
//             atomics, one set per horizontal run of foreground pixels within a wave's 64 columns of one image row; the same pass
//             measures a label image (one row per label, a run = equal neighbouring labels)
//   shape     of a label image: the inner boundary of every object as a map, and per label the second moments about the corner of
//             its bounding box and four tallies of its boundary pixels by neighbourhood class (the perimeter estimate's weights) --
//             a walk of measure's kind, integer atomics per run
//   quantify  of a label image over an RGB image: per label (and per ring of an expanded label image) the integer stain levels of
//             its pixels -- count, sum, sum of squares, maximum, positive pixels, histogram; the same walk again
//   hull      of a label image: per label the convex hull of its pixels' unit squares -- vertex count, twice the area, the largest
//             squared vertex distance and the smallest width as an exact fraction; one workgroup per label, the row extents of its
//             bounding box and the hull's vertices in LDS, no atomics and no workspace
//   contour   of a label image: per label the outer boundary of its first component as an ordered ring of lattice vertices, with
//             the ring's crack count and enclosed area and the crack count of the whole label; one workgroup per label, its
//             bounding box as a bitmap in LDS, which one thread walks
//   texture   of a label image over a uint8 plane or one stain of an RGB image: per label and per direction (0, 45, 90, 135
//             degrees at one distance) the grey-level co-occurrence matrix of the pixel pairs inside the label, folded to its pair
//             count, difference, sum and marginal histograms, sum of squares and cross moment; one workgroup per label, four
//             L x L tables of counters in LDS, no global atomics and no workspace
//   match     a label image against another: per-label areas of both, and for every pred label the one truth label with
//             IoU > 1/2, if any -- two walks of measure's kind (bit votes spell the candidate, then its intersection is counted)
//             and an exact 64-bit integer test per pred label
//   overlap   the same two images: every (pred, truth) pair that shares a pixel with its count, in a per-image hash table filled by
//             one walk, and from it every label's partner of largest IoU / largest intersection (integer maxima under a total order)
//   adjacency one label image against its own shifted self: every pair of labels that shares a pixel side (or corner) with the
//             counts, in overlap's hash table filled by one walk over three rows at a time, per label the sides shared with other
//             labels, with the background and with the image edge, and the neighbour of longest contact; seed_labels paints a
//             ragged point set into the label image that the Voronoi graph of the points is read from
//   hausdorff the same two images and overlap's partners: the squared Hausdorff distance of every object to its partner, one
//             workgroup per pair, the target's horizontal runs staged in LDS and every pixel of the source held against them
//   split     every foreground pixel goes to the nearest seed point of ITS OWN component (squared distance, then seed index), a
//             component without a seed is numbered after the seeds:
//               seeds   one thread per row of the ragged point set (cs_points.h) hangs the live seeds on a chain at their
//                       component's root
//               number  the numbering trio over the roots that have no seed
//               assign  every pixel walks the chain of its root; a wave whose foreground lanes share a root walks it as one
//   geodesic  the same split with the distance measured along paths that stay inside the component (5-7 chamfer steps), so that
//             every cell is connected: one 64-bit key (distance, seed) per pixel, lowered to its fixpoint by rounds of one launch
//             each in which every 64 x 64 tile relaxes in LDS against a one-pixel halo; a byte per tile and round skips the tiles
//             where nothing can change any more
// Hooks only ever lower a label and a label is always an index of the same component, so the root of a component is its lowest
// index whatever order the hooks land in; areas are integer sums.  The result does not depend on launch order.  Every union loop
// lowers max(a, b) in each turn that does not end it, so it is bounded by the index range; nothing waits on another thread.
// The number of launches depends on (N, H, W) only (for a split also on whether there is any point, for a geodesic split also on
// the number of rounds asked for) and nothing synchronises with the host.
#include <limits.h>
#include <stdio.h>
#include "cs_common.h"
#include "cs_block.h"
#include "cs_points.h"

namespace {

constexpr int kT = 64;                 // tile edge
constexpr int kTP = kT * kT;           // pixels per tile
constexpr int kPer = kTP / 256;        // pixels per thread of the tile kernel
constexpr int kNB = 1024;              // pixels per block of the numbering kernels

constexpr int kLds = __HIP_MEMORY_SCOPE_WORKGROUP, kGlobal = __HIP_MEMORY_SCOPE_AGENT;   // where the labels of a union-find live

// grid (tiles across, tiles down, N).  val: 0 / 1 = the pixel's value, 2 = outside the image.
template <int CONN>
__global__ __launch_bounds__(256) void tile_label_kernel(const uint8_t* __restrict__ m, int H, int W, int32_t* __restrict__ lab_g,
                                                         int32_t* __restrict__ cnt_g) {
    __shared__ int lab[kTP];
    __shared__ int cnt[kTP];
    __shared__ uint8_t val[kTP];
    const int c0 = blockIdx.x * kT, r0 = blockIdx.y * kT;
    const long long img = (long long)blockIdx.z * H * W;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int r = r0 + (i >> 6), c = c0 + (i & 63);
        val[i] = (r < H && c < W) ? (uint8_t)(m[img + (long long)r * W + c] != 0) : (uint8_t)2;
        lab[i] = i;
        cnt[i] = 0;
    }
    __syncthreads();
    for (int k = 0; k < kPer; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int ly = i >> 6, lx = i & 63;
        const int v = val[i];
        if (v == 2) continue;
        if (lx > 0 && val[i - 1] == v) uf_unite<kLds>(lab, i, i - 1);
        if (ly > 0) {
            if (val[i - kT] == v) uf_unite<kLds>(lab, i, i - kT);
            if (CONN == 2) {
                if (lx > 0 && val[i - kT - 1] == v) uf_unite<kLds>(lab, i, i - kT - 1);
                if (lx < kT - 1 && val[i - kT + 1] == v) uf_unite<kLds>(lab, i, i - kT + 1);
            }
        }
    }
    __syncthreads();
    int root[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = threadIdx.x + 256 * k;
        root[k] = val[i] == 2 ? -1 : uf_find<kLds>(lab, i);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        // a wave covers one tile row: where the whole row lies in one component, one add of 64 instead of 64 adds of 1
        const int first = __builtin_amdgcn_readfirstlane(root[k]);
        if (__all(root[k] == first)) {
            if (first >= 0 && (threadIdx.x & 63) == 0) atomicAdd(cnt + first, 64);
        } else if (root[k] >= 0) {
            atomicAdd(cnt + root[k], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (root[k] < 0) continue;
        const int i = threadIdx.x + 256 * k;
        const long long p = img + (long long)(r0 + (i >> 6)) * W + c0 + (i & 63);
        lab_g[p] = (int32_t)(img + (long long)(r0 + (root[k] >> 6)) * W + c0 + (root[k] & 63));
        cnt_g[p] = root[k] == i ? cnt[i] : 0;
    }
}

// One thread per pixel of every tile's first row (rows 64, 128, ...) and first column (columns 64, 128, ...).
template <int CONN>
__global__ __launch_bounds__(256) void border_kernel(const uint8_t* __restrict__ m, int N, int H, int W, int32_t* __restrict__ lab) {
    const long long n_row = (long long)((H - 1) / kT) * W, n_col = (long long)((W - 1) / kT) * H;
    const long long per = n_row + n_col, total = per * N;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const long long n = g / per;
        long long e = g - n * per;
        const long long base = n * H * W;
        auto join = [&](long long p, long long q, bool v) {
            if ((m[q] != 0) == v) uf_unite<kGlobal>(lab, (int)p, (int)q);
        };
        if (e < n_row) {
            const int r = ((int)(e / W) + 1) * kT, c = (int)(e % W);
            const long long p = base + (long long)r * W + c;
            const bool v = m[p] != 0;
            join(p, p - W, v);
            if (CONN == 2) {
                if (c > 0) join(p, p - W - 1, v);
                if (c < W - 1) join(p, p - W + 1, v);
            }
        } else {
            e -= n_row;
            const int c = ((int)(e / H) + 1) * kT, r = (int)(e % H);
            const long long p = base + (long long)r * W + c;
            const bool v = m[p] != 0;
            join(p, p - 1, v);
            if (CONN == 2) {
                if (r > 0) join(p, p - W - 1, v);
                if (r < H - 1) join(p, p + W - 1, v);
            }
        }
    }
}

// lab[p] = root; the count a tile left at p moves to the root's slot (nothing is ever added to a slot that is not a root)
__global__ __launch_bounds__(256) void flatten_kernel(long long total, int32_t* __restrict__ lab, int32_t* __restrict__ cnt) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const int root = uf_find<kGlobal>(lab, (int)p);
        __hip_atomic_store(lab + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c = cnt[p];
        if (c != 0 && root != (int)p) atomicAdd(cnt + root, c);
    }
}

__global__ __launch_bounds__(256) void filter_kernel(const uint8_t* m, long long total, const int32_t* __restrict__ lab,
                                                     const int32_t* __restrict__ cnt, int value, int min_area, uint8_t* out) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const int v = m[p] != 0;
        out[p] = (uint8_t)((v == value && cnt[lab[p]] < min_area) ? 1 - value : v);
    }
}

__global__ __launch_bounds__(256) void spread_kernel(const uint8_t* __restrict__ m, long long total, const int32_t* __restrict__ lab,
                                                     const int32_t* __restrict__ table, int foreground_only, int32_t* __restrict__ out) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256)
        out[p] = (foreground_only && m[p] == 0) ? 0 : table[lab[p]];
}

// ---- the seed points of a split: the ragged point set of cs_points.h, rows (row, col); off == NULL (P == 0) = no seeds at all ------
// S'_n, the number of points of image n that are seeds: the rows its window keeps
__device__ __forceinline__ int seed_limit(const PointSet& s, int n) { return s.off ? point_window(s, n).kept : 0; }

// ---- scipy's numbering: grid (blocks per image, N), kNB pixels per block --------------------------------------------------------
// SEEDLESS = false: every foreground root.  SEEDLESS = true (split): the foreground roots whose slot of `cnt` still holds the area
// that label_into left there (> 0); the seed pass has replaced it by a chain head (< 0) at every root that has a live seed.
template <bool SEEDLESS>
__device__ __forceinline__ bool is_fg_root(const uint8_t* m, const int32_t* lab, const int32_t* cnt, long long HW, long long i,
                                           long long base) {
    return i < HW && m[base + i] != 0 && lab[base + i] == (int32_t)(base + i) && (!SEEDLESS || cnt[base + i] > 0);
}

template <bool SEEDLESS>
__global__ __launch_bounds__(kNB) void number_count_kernel(const uint8_t* __restrict__ m, const int32_t* __restrict__ lab,
                                                           const int32_t* __restrict__ cnt, long long HW, int32_t* __restrict__ blk) {
    __shared__ int wsum[kNB / 64];
    const long long i = (long long)blockIdx.x * kNB + threadIdx.x;
    int total;
    block_rank<kNB>(is_fg_root<SEEDLESS>(m, lab, cnt, HW, i, blockIdx.y * HW), wsum, total);
    if (threadIdx.x == 0) blk[(long long)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one workgroup per image: blk[n][0..B) -> its exclusive prefix sums, in place
// counts (or NULL): [n] = the number of counted roots of image n, after its seeds_n = S'_n seeds
__global__ __launch_bounds__(1024) void number_scan_kernel(int32_t* __restrict__ blk_all, int B, int32_t* __restrict__ counts, PointSet seeds) {
    __shared__ int part[1024];
    int32_t* blk = blk_all + (long long)blockIdx.x * B;
    const int seg = (B + 1023) / 1024;
    const int lo = min((int)threadIdx.x * seg, B), hi = min(lo + seg, B);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += blk[i];
    int total;
    int run = block_scan_incl<1024>(s, part, total) - s;
    if (counts && threadIdx.x == 0) counts[blockIdx.x] = seed_limit(seeds, blockIdx.x) + total;
    for (int i = lo; i < hi; ++i) {
        const int v = blk[i];
        blk[i] = run;
        run += v;
    }
}

// num: the cnt array itself -- a counted root reads its own slot (SEEDLESS) and then writes its number there, nobody else's
template <bool SEEDLESS>
__global__ __launch_bounds__(kNB) void number_assign_kernel(const uint8_t* __restrict__ m, const int32_t* __restrict__ lab, long long HW,
                                                            const int32_t* __restrict__ blk, int32_t* num, PointSet seeds) {
    __shared__ int wsum[kNB / 64];
    const long long base = blockIdx.y * HW;
    const long long i = (long long)blockIdx.x * kNB + threadIdx.x;
    const bool root = is_fg_root<SEEDLESS>(m, lab, num, HW, i, base);
    int total;
    const int before = block_rank<kNB>(root, wsum, total);
    if (!root) return;
    num[base + i] = seed_limit(seeds, blockIdx.y) + blk[(long long)blockIdx.y * gridDim.x + blockIdx.x] + before + 1;
}

// ---- one table row per component: row (n, k) of every table belongs to the component numbered k + 1 of image n ------------------
struct Tables {
    int32_t* area;       // [N][cap]
    int32_t* bbox;       // [N][cap][4] = r0, c0, r1, c1 (half-open)
    long long* sums;     // [N][cap][2] = sum of rows, sum of columns
    long long* isum;     // [N][cap], with an intensity image
    int32_t* imax;       // [N][cap], with an intensity image
};

// All zero, except that the lower bounds of the rows that will be written (k < count) start at INT_MAX: every such component has
// a pixel, so none of them is left behind.  counts = NULL (a label image: a label below the count may own no pixel): every lower
// bound starts at INT_MAX and measure_empty_rows_kernel puts the rows that stayed empty right; maxlab [N] is then zeroed for the
// label maxima.
__global__ __launch_bounds__(256) void measure_init_kernel(const int32_t* __restrict__ counts, int N, int cap, Tables t, int with_v,
                                                           int32_t* __restrict__ maxlab) {
    const long long rows = (long long)N * cap;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const int lo = (!counts || (int)(i % cap) < counts[i / cap]) ? INT_MAX : 0;
        if (maxlab && i < N) maxlab[i] = 0;
        t.area[i] = 0;
        t.bbox[4 * i] = lo;
        t.bbox[4 * i + 1] = lo;
        t.bbox[4 * i + 2] = 0;
        t.bbox[4 * i + 3] = 0;
        t.sums[2 * i] = 0;
        t.sums[2 * i + 1] = 0;
        if (with_v) {
            t.isum[i] = 0;
            t.imax[i] = 0;
        }
    }
}

// min / max into a slot that only ever moves one way: a value read earlier in this launch is never beyond the current one, so an
// update that the read value already covers is dropped without an atomic, however stale the read is.
__device__ __forceinline__ void lower_to(int32_t* p, int x) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, kGlobal) > x) __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, kGlobal);
}
__device__ __forceinline__ void raise_to(int32_t* p, int x) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, kGlobal) < x) __hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, kGlobal);
}

// the rows of a label image's tables that no pixel wrote (a label that owns nothing, e.g. the second of two seeds on one pixel):
// all zero, as the rows beyond the count
__global__ __launch_bounds__(256) void measure_empty_rows_kernel(long long rows, Tables t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        if (t.area[i] != 0) continue;
        t.bbox[4 * i] = 0;
        t.bbox[4 * i + 1] = 0;
    }
}

// The runs of a wave's 64 lanes.  live: the lanes that belong to a run at all; breaks: live lanes that start a new run although
// the lane to their left is live too.  A run also starts where the lane to the left is not live, and at lane 0.  Returns whether
// this lane is the head of its run; len = the lanes from this one to its run's last (1 on a lane that is not live).
__device__ __forceinline__ bool run_of(unsigned long long live, unsigned long long breaks, int lane, int& len) {
    const unsigned long long start = (live & ~(live << 1)) | breaks;
    const unsigned long long rest = ((~live | start) >> lane) >> 1;    // bit i = lane + 1 + i is no part of this lane's run
    len = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
    return (start >> lane) & 1;
}

// The walk of every kernel that works on horizontal runs: over (image, row, 64-column segment) items, one wave per item, four per
// workgroup of 256 threads (grid: walk_grid(N, H, W)).  body(n, r, c, p): image n, row r, column c = 64 segment + lane, pixel index
// p = (n H + r) W + c.  A wave takes 64 consecutive columns of ONE image row, so it never straddles a row end; n and r are
// wave-uniform, and the body is called with the WHOLE wave, the lanes with c >= W included (p is then no pixel of that row), so it
// may ballot and shuffle.  `return` in the body ends the item (by the whole wave where a ballot or shuffle would still follow).
template <typename Body>
__device__ __forceinline__ void walk_row_segments(int N, int H, int W, Body body) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned segs = (unsigned)(W + 63) >> 6;
    const long long items = (long long)N * H * segs;                   // <= N H W < 2^31
    for (long long it = (long long)blockIdx.x * 4 + wave; it < items; it += (long long)gridDim.x * 4) {
        const unsigned row = (unsigned)it / segs;                      // n H + r
        const int c = (int)((unsigned)it - row * segs) * 64 + lane;
        const int n = (int)(row / (unsigned)H), r = (int)(row - (unsigned)n * (unsigned)H);
        body(n, r, c, (long long)row * W + c);
    }
}

// Horizontal neighbours in the foreground are one component, so a maximal run of foreground lanes has one table row: its head
// lane looks the number up once and issues one set of atomics for the whole run -- length, closed-form column sum, and the
// intensity sum / maximum from a segmented shuffle reduction.  lab: every pixel's root; num: every foreground root's number.
// LABELS: lab is a label image instead (m and num are not read): foreground = a positive label, table row = label - 1, and a run
// also starts where the label differs from the left neighbour's -- neighbouring foreground pixels may belong to different cells.
// The head lanes also raise maxlab[n] (or NULL) to their label.
template <bool LABELS>
__global__ __launch_bounds__(256) void measure_kernel(const uint8_t* __restrict__ m, const uint8_t* __restrict__ v, int N, int H, int W,
                                                      const int32_t* __restrict__ lab, const int32_t* __restrict__ num, int cap, Tables t,
                                                      int32_t* __restrict__ maxlab) {
    const int lane = threadIdx.x & 63;
    const long long total = (long long)N * H * W;
    walk_row_segments(N, H, W, [&](int n, int r, int c, long long p) {
        const int l = (LABELS && c < W) ? lab[p] : 0;
        const bool fg = LABELS ? l > 0 : (c < W && m[p] != 0);
        const unsigned long long bal = __ballot(fg);
        if (bal == 0) return;
        int s = (v && fg) ? v[p] : 0, mx = s;
        int len;
        // LABELS: a run also breaks where the lane carries another label than its left neighbour (lane 0 gets its own back)
        const bool head = run_of(bal, LABELS ? __ballot(fg && l != __shfl_up(l, 1)) : 0ull, lane, len);
        if (v) {
            const int last = fg ? lane + len - 1 : lane;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {                   // lane i: the sum / maximum over [i, min(i + 2 off - 1, last)]
                const int os = __shfl_down(s, off), om = __shfl_down(mx, off);
                if (lane + off <= last) {
                    s += os;
                    mx = max(mx, om);
                }
            }
        }
        if (!head) return;
        int k;
        if (LABELS) {
            k = l - 1;
            if (maxlab) raise_to(maxlab + n, l);
        } else {
            const int root = lab[p];
            if ((unsigned)root >= (unsigned)total) return;             // never with a workspace that label_into filled
            k = num[root] - 1;
        }
        if ((unsigned)k >= (unsigned)cap) return;
        const long long q = (long long)n * cap + k;
        __hip_atomic_fetch_add(t.area + q, len, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_add(t.sums + 2 * q, (long long)r * len, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_add(t.sums + 2 * q + 1, (long long)len * c + (long long)len * (len - 1) / 2, __ATOMIC_RELAXED, kGlobal);
        lower_to(t.bbox + 4 * q, r);
        lower_to(t.bbox + 4 * q + 1, c);
        raise_to(t.bbox + 4 * q + 2, r + 1);
        raise_to(t.bbox + 4 * q + 3, c + len);
        if (v) {
            __hip_atomic_fetch_add(t.isum + q, (long long)s, __ATOMIC_RELAXED, kGlobal);
            raise_to(t.imax + q, mx);
        }
    });
}

// ---- the shape of every label: inner boundary, second moments, perimeter tallies --------------------------------------------------
// A pixel's object id is max(label, 0).  An edge pixel has a positive id and a 4-neighbour of another id (outside the image: 0):
// the object minus its erosion by the 4-neighbourhood, per object.  A wave reads its 64 columns of rows r - 1, r, r + 1; the ids
// left and right come by shuffle, at lanes 0 and 63 from the columns across the segment's ends.
__global__ __launch_bounds__(256) void edge_kernel(const int32_t* __restrict__ lab, int N, int H, int W, uint8_t* __restrict__ edges) {
    const int lane = threadIdx.x & 63;
    walk_row_segments(N, H, W, [&](int, int r, int c, long long p) {
        const bool in = c < W;
        const int l = in ? max(lab[p], 0) : 0;
        int left = __shfl_up(l, 1), right = __shfl_down(l, 1);         // a lane with c >= W carries 0: the id outside the image
        if (lane == 0) left = c > 0 ? max(lab[p - 1], 0) : 0;
        if (lane == 63) right = c + 1 < W ? max(lab[p + 1], 0) : 0;
        if (!in) return;
        bool edge = false;
        if (l > 0) {
            const int up = r > 0 ? max(lab[p - W], 0) : 0, down = r < H - 1 ? max(lab[p + W], 0) : 0;
            edge = left != l || right != l || up != l || down != l;
        }
        edges[p] = (uint8_t)edge;
    });
}

struct ShapeTables {
    const int32_t* bbox;     // [N][cap][4], read: the origin (r0, c0) of every label's moments
    long long* moments;      // [N][cap][3] = Sxx, Syy, Sxy with x = r - r0, y = c - c0
    int32_t* tallies;        // [N][cap][4] = edge pixels, straight, diagonal, mixed
};

__global__ __launch_bounds__(256) void shape_init_kernel(long long rows, ShapeTables t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 4 * rows; i += (long long)gridDim.x * 256) {
        t.tallies[i] = 0;
        if (i < 3 * rows) t.moments[i] = 0;
    }
}

// lane i: the sum of s over the lanes [i, last] of its run, last = the run's last lane (the lane itself where it is in no run)
__device__ __forceinline__ int run_sum(int s, int lane, int last) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                           // lane i: the sum over [i, min(i + 2 off - 1, last)]
        const int o = __shfl_down(s, off);
        if (lane + off <= last) s += o;
    }
    return s;
}

// An edge pixel of object l with n4 of its 4-neighbours and nd of its diagonal neighbours edge pixels of l too has the code
// 1 + 2 n4 + 10 nd (< 64), and the code its class: bit `code` of these masks.
constexpr unsigned long long kStraight = 1ull << 5 | 1ull << 7 | 1ull << 15 | 1ull << 17 | 1ull << 25 | 1ull << 27;
constexpr unsigned long long kDiagonal = 1ull << 21 | 1ull << 33;
constexpr unsigned long long kMixed = 1ull << 13 | 1ull << 23;

// The runs of measure_kernel<true>: per run one set of int64 adds for the moments in closed form, and one add per tally that is
// not zero.  el = the "edge id" of a pixel: its id where it is an edge pixel, else 0 -- a neighbour counts iff its edge id is l.
// The four tallies of a lane travel through the segmented reduction as the bytes of one int (a run has at most 64 pixels).
__global__ __launch_bounds__(256) void shape_kernel(const int32_t* __restrict__ lab, const uint8_t* __restrict__ edges, int N, int H, int W,
                                                    int cap, ShapeTables t) {
    const int lane = threadIdx.x & 63;
    walk_row_segments(N, H, W, [&](int n, int r, int c, long long p) {
        const bool in = c < W;
        const int l = in ? max(lab[p], 0) : 0;
        const unsigned long long bal = __ballot(l > 0);
        if (bal == 0) return;
        auto edge_id = [&](long long q) { return edges[q] ? max(lab[q], 0) : 0; };
        const int el = (l > 0 && edges[p]) ? l : 0;
        int packed = 0;
        if (__ballot(el != 0)) {                                       // wave-uniform: the shuffles below are made by all lanes
            const bool above = r > 0, below = r < H - 1;
            const int eu = (in && above) ? edge_id(p - W) : 0, ed = (in && below) ? edge_id(p + W) : 0;
            int lu = __shfl_up(eu, 1), lm = __shfl_up(el, 1), ld = __shfl_up(ed, 1);
            int ru = __shfl_down(eu, 1), rm = __shfl_down(el, 1), rd = __shfl_down(ed, 1);
            if (lane == 0) {
                const bool has = c > 0;
                lm = has ? edge_id(p - 1) : 0;
                lu = (has && above) ? edge_id(p - W - 1) : 0;
                ld = (has && below) ? edge_id(p + W - 1) : 0;
            }
            if (lane == 63) {
                const bool has = c + 1 < W;
                rm = has ? edge_id(p + 1) : 0;
                ru = (has && above) ? edge_id(p - W + 1) : 0;
                rd = (has && below) ? edge_id(p + W + 1) : 0;
            }
            if (el) {
                const int n4 = (lm == l) + (rm == l) + (eu == l) + (ed == l), nd = (lu == l) + (ru == l) + (ld == l) + (rd == l);
                const int code = 1 + 2 * n4 + 10 * nd;
                packed = 1 | (int)((kStraight >> code) & 1) << 8 | (int)((kDiagonal >> code) & 1) << 16 | (int)((kMixed >> code) & 1) << 24;
            }
        }
        int len;
        const bool head = run_of(bal, __ballot(l > 0 && l != __shfl_up(l, 1)), lane, len);
        packed = run_sum(packed, lane, l > 0 ? lane + len - 1 : lane);
        if (!head || l > cap) return;
        const long long q = (long long)n * cap + l - 1;
        const long long x = r - t.bbox[4 * q], y = c - t.bbox[4 * q + 1], m = len;   // the run: row x, columns y .. y + m - 1
        const long long tri = m * (m - 1) / 2;                         // sum of j, j < m; sum of j^2 = tri (2 m - 1) / 3
        __hip_atomic_fetch_add(t.moments + 3 * q, m * x * x, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_add(t.moments + 3 * q + 1, m * y * y + 2 * y * tri + tri * (2 * m - 1) / 3, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_add(t.moments + 3 * q + 2, x * (m * y + tri), __ATOMIC_RELAXED, kGlobal);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int add = (packed >> (8 * k)) & 0xFF;
            if (add) __hip_atomic_fetch_add(t.tallies + 4 * q + k, add, __ATOMIC_RELAXED, kGlobal);
        }
    });
}

// ---- how strongly every label is stained: integer stain levels of an RGB image, tabulated per (label, compartment) -----------------
// A pixel belongs to (row labels[p] - 1, compartment 0) where labels[p] > 0, else to (row expanded[p] - 1, compartment 1) where
// there is an expanded image and expanded[p] > 0, else to nothing.  Its level of stain s is
//   clamp((Mq[n][s][0] od_q[R] + Mq[n][s][1] od_q[G] + Mq[n][s][2] od_q[B] + 2^23) >> 24, 0, 255)      (int64, arithmetic shift),
// at most 2^31 * 22713 * 3 + 2^23 < 2^48 in magnitude.  Per (image, row, compartment) n, and per stain the sum, the sum of squares,
// the maximum of the level, the pixels with level >= pos_level[s], and with bins > 0 the pixels per bin = level * bins >> 8.
struct QuantTables {
    int32_t* n;          // [N][cap][C]
    long long* sum;      // [N][cap][C][K]
    long long* sumsq;    // [N][cap][C][K]
    int32_t* mx;         // [N][cap][C][K]
    int32_t* pos;        // [N][cap][C][K]
    int32_t* hist;       // [N][cap][C][K][bins], bins > 0
    int32_t* maxlab;     // [N] or NULL
    int C, bins;
    int pos_level[3];    // 256 = no pixel is positive
};

__global__ __launch_bounds__(256) void quantify_init_kernel(long long slots, int K, int N, QuantTables t) {
    const long long cells = slots * K, all = t.bins ? cells * t.bins : cells;      // >= slots >= N
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long long)gridDim.x * 256) {
        if (t.bins) t.hist[i] = 0;
        if (i < cells) {
            t.sum[i] = 0;
            t.sumsq[i] = 0;
            t.mx[i] = 0;
            t.pos[i] = 0;
        }
        if (i < slots) t.n[i] = 0;
        if (i < N && t.maxlab) t.maxlab[i] = 0;
    }
}

// The runs of measure_kernel<true>, a run being a stretch of lanes with the same (row, compartment): id = the label for
// compartment 0, minus the label for compartment 1, 0 where the pixel belongs to nothing.  Every lane reads the three bytes of its
// own pixel, so nothing is asked of the image's alignment; a wave's loads cover 192 consecutive bytes.  Per stain three ints go
// through the segmented reduction: sum | positives << 16 (a run has at most 64 pixels: 64 * 255 < 2^16), the sum of squares
// (64 * 255^2 < 2^23) and the maximum.  The head lane adds them with one atomic each; the histogram is added per pixel.
template <int K>
__global__ __launch_bounds__(256) void quantify_kernel(const uint8_t* __restrict__ rgb, const int32_t* __restrict__ lab,
                                                       const int32_t* __restrict__ expd, int N, int H, int W,
                                                       const int32_t* __restrict__ od_q, const int32_t* __restrict__ Mq, int cap, QuantTables t) {
    __shared__ int32_t s_od[256];
    s_od[threadIdx.x] = od_q[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    walk_row_segments(N, H, W, [&](int n, int r, int c, long long p) {
        const bool in = c < W;
        int id = in ? max(lab[p], 0) : 0;
        if (expd && in && id == 0) id = -max(expd[p], 0);
        const unsigned long long bal = __ballot(id != 0);
        if (bal == 0) return;
        const int l = id < 0 ? -id : id, comp = id < 0;
        const bool measured = id != 0 && l <= cap;
        const long long slot = ((long long)n * cap + l - 1) * t.C + comp;  // used where `measured` only
        int a[K], b[K], m[K];
#pragma unroll
        for (int s = 0; s < K; ++s) a[s] = b[s] = m[s] = 0;
        if (measured) {
            const uint8_t* px = rgb + 3 * p;
            const long long qr = s_od[px[0]], qg = s_od[px[1]], qb = s_od[px[2]];
            const int32_t* mq = Mq + (long long)n * K * 3;
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const long long acc = mq[3 * s] * qr + mq[3 * s + 1] * qg + mq[3 * s + 2] * qb + (1LL << 23);
                const long long sh = acc >> 24;
                const int lv = (int)(sh < 0 ? 0 : sh > 255 ? 255 : sh);
                a[s] = lv | (int)(lv >= t.pos_level[s]) << 16;
                b[s] = lv * lv;
                m[s] = lv;
                if (t.bins) __hip_atomic_fetch_add(t.hist + ((slot * K + s) * t.bins + ((lv * t.bins) >> 8)), 1, __ATOMIC_RELAXED, kGlobal);
            }
        }
        int len;
        const bool head = run_of(bal, __ballot(id != 0 && id != __shfl_up(id, 1)), lane, len);
        const int last = id != 0 ? lane + len - 1 : lane;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {                       // lane i: over [i, min(i + 2 off - 1, last)]
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const int oa = __shfl_down(a[s], off), ob = __shfl_down(b[s], off), om = __shfl_down(m[s], off);
                if (lane + off <= last) {
                    a[s] += oa;
                    b[s] += ob;
                    m[s] = max(m[s], om);
                }
            }
        }
        if (!head) return;
        if (t.maxlab) raise_to(t.maxlab + n, l);
        if (!measured) return;
        __hip_atomic_fetch_add(t.n + slot, len, __ATOMIC_RELAXED, kGlobal);
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const long long q = slot * K + s;
            const int sum = a[s] & 0xFFFF, pos = a[s] >> 16;
            if (sum) __hip_atomic_fetch_add(t.sum + q, (long long)sum, __ATOMIC_RELAXED, kGlobal);
            if (b[s]) __hip_atomic_fetch_add(t.sumsq + q, (long long)b[s], __ATOMIC_RELAXED, kGlobal);
            if (pos) __hip_atomic_fetch_add(t.pos + q, pos, __ATOMIC_RELAXED, kGlobal);
            raise_to(t.mx + q, m[s]);
        }
    });
}

// ---- the convex hull of every label: vertex count, area, largest and smallest Feret diameter ---------------------------------------
// An object is the union of the closed unit squares of its pixels; in lattice coordinates relative to the corner of its box,
// pixel (i, j) has the corners (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1).  On lattice row r lie the corners of the pixel rows
// r - 1 and r, and only the leftmost and the rightmost of them can be vertices of the hull: the left chain runs down the leftmost
// points, the right chain down the rightmost, and the hull is the left chain followed by the right chain backwards.  The ends of
// the chains are the ends of the top and the bottom edge, which are horizontal and at least one pixel long.
constexpr int kHullSide = 1024;        // cs_regions_hull_max_side: coordinates <= 1024, cross products <= 2^21, squared ones <= 2^42
constexpr int kHullNone = 0xFFFF;      // lo of a pixel row without a pixel of the label (its hi is 0)

struct HullLds {
    uint16_t lo[kHullSide], hi[kHullSide];   // per pixel row of the box: the leftmost column of the label, the rightmost + 1
    // Every lattice row gives one candidate per chain, so a box of `rows` pixel rows has at most 2 (rows + 1) hull vertices:
    // rows + 1 <= kHullSide + 1 per chain.  A vertex is r << 16 | c.  12.3 KiB with lo and hi.
    int32_t chain[2][kHullSide + 1];
    int n[2];
    long long red[4];
};

// the narrower of two edges (cross << 32 | len2; below 0: none): the smaller cross^2 / len2, then the smaller len2.  The products
// are below 2^42 2^21 = 2^63.
__device__ __forceinline__ long long hull_narrower(long long a, long long b) {
    if (a < 0 || b < 0) return a < 0 ? b : a;
    const unsigned long long ca = (unsigned long long)a >> 32, la = (unsigned long long)a & 0xFFFFFFFFull;
    const unsigned long long cb = (unsigned long long)b >> 32, lb = (unsigned long long)b & 0xFFFFFFFFull;
    const unsigned long long wa = ca * ca * lb, wb = cb * cb * la;
    if (wa != wb) return wa < wb ? a : b;
    return la <= lb ? a : b;
}

// One workgroup per (image, label) at a time.  The box is cut to the image before anything is read, so whatever the table holds
// no read leaves the label image.
__global__ __launch_bounds__(256) void hull_kernel(const int32_t* __restrict__ lab, int N, int H, int W, int cap,
                                                   const int32_t* __restrict__ bbox, int32_t* __restrict__ hull) {
    __shared__ HullLds s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long objects = (long long)N * cap;
    for (long long q = blockIdx.x; q < objects; q += gridDim.x) {
        const int n = (int)(q / cap), l = (int)(q - (long long)n * cap) + 1;
        const int r0 = max(bbox[4 * q], 0), c0 = max(bbox[4 * q + 1], 0);
        const int rows = min(bbox[4 * q + 2], H) - r0, cols = min(bbox[4 * q + 3], W) - c0;
        const bool none = rows <= 0 || cols <= 0;
        if (none || rows > kHullSide || cols > kHullSide) {            // the same in every thread: no barrier is left out below
            if (threadIdx.x < 5) hull[5 * q + threadIdx.x] = none ? 0 : -1;
            continue;
        }
        // 1. the extents of every pixel row: a wave per row, its lanes stride over the columns of the box
        const int32_t* img = lab + (long long)n * H * W + (long long)r0 * W + c0;
        for (int i = wave; i < rows; i += 4) {
            const int32_t* row = img + (long long)i * W;
            int lo = kHullNone, hi = 0;
            for (int c = lane; c < cols; c += 64) {
                if (row[c] == l) {
                    lo = min(lo, c);
                    hi = c + 1;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lo = min(lo, __shfl_xor(lo, off));
                hi = max(hi, __shfl_xor(hi, off));
            }
            if (lane == 0) {
                s.lo[i] = (uint16_t)lo;
                s.hi[i] = (uint16_t)hi;
            }
        }
        __syncthreads();
        // 2. the two chains, each by one thread of a wave of its own: a streaming stack over the lattice rows, top to bottom.  With
        //    a the vertex below the top b and p the candidate, b stays while it lies strictly outside the line a -> p.
        if (lane == 0 && wave < 2) {
            const bool right = wave == 1;
            int32_t* v = s.chain[wave];
            int m = 0;
            for (int r = 0; r <= rows; ++r) {
                int c;
                if (right) {
                    c = max(r > 0 ? (int)s.hi[r - 1] : 0, r < rows ? (int)s.hi[r] : 0);
                    if (c == 0) continue;
                } else {
                    c = min(r > 0 ? (int)s.lo[r - 1] : kHullNone, r < rows ? (int)s.lo[r] : kHullNone);
                    if (c == kHullNone) continue;
                }
                while (m >= 2) {
                    const int a = v[m - 2], b = v[m - 1];
                    const int ar = a >> 16, ac = a & 0xFFFF;
                    const int turn = ((b >> 16) - ar) * (c - ac) - ((b & 0xFFFF) - ac) * (r - ar);
                    if (right ? turn < 0 : turn > 0) break;
                    --m;
                }
                v[m++] = r << 16 | c;
            }
            s.n[wave] = m;
        }
        __syncthreads();
        // 3. a thread per edge a -> b, every vertex held against it: the farthest from a, and the farthest from the edge's line
        const int nl = s.n[0], nr = s.n[1], V = nl + nr;
        auto vertex = [&](int k) { return k < nl ? s.chain[0][k] : s.chain[1][V - 1 - k]; };
        long long area2 = 0, far2 = 0, narrow = -1;
        for (int k = threadIdx.x; k < V; k += 256) {
            const int a = vertex(k), b = vertex(k + 1 == V ? 0 : k + 1);
            const int ar = a >> 16, ac = a & 0xFFFF, br = b >> 16, bc = b & 0xFFFF, er = br - ar, ec = bc - ac;
            area2 += ar * bc - br * ac;
            int cross = 0, d2 = 0;
            for (int side = 0; side < 2; ++side) {
                const int count = side ? nr : nl;
                for (int j = 0; j < count; ++j) {
                    const int p = s.chain[side][j];
                    const int dr = (p >> 16) - ar, dc = (p & 0xFFFF) - ac;
                    cross = max(cross, abs(er * dc - ec * dr));
                    d2 = max(d2, dr * dr + dc * dc);
                }
            }
            far2 = max(far2, (long long)d2);
            narrow = hull_narrower(narrow, (long long)cross << 32 | (long long)(er * er + ec * ec));
        }
        area2 = block_reduce<256>(area2, [](long long x, long long y) { return x + y; }, s.red);
        far2 = block_reduce<256>(far2, [](long long x, long long y) { return x > y ? x : y; }, s.red);
        // (the last barrier of this call is the one after which the next object may overwrite s)
        narrow = block_reduce<256>(narrow, [](long long x, long long y) { return hull_narrower(x, y); }, s.red);
        if (threadIdx.x == 0) {
            int32_t* out = hull + 5 * q;
            out[0] = V;
            out[1] = (int)(area2 < 0 ? -area2 : area2);
            out[2] = (int)far2;
            out[3] = narrow < 0 ? 0 : (int)(narrow >> 32);
            out[4] = narrow < 0 ? 0 : (int)(narrow & 0xFFFFFFFFll);
        }
    }
}

// ---- the outer boundary ring of every label: an ordered polygon of lattice vertices ---------------------------------------------
// The object of label l is the pixels with id l inside its box, pixel (i, j) of the box being the closed unit square with the
// lattice corners (i, j) and (i + 1, j + 1).  A crack is one unit side of a pixel of the object whose neighbour across it is not in
// the object; walked with the object on the right hand, every crack has exactly one successor (the rule is at `contour_walk`), so
// the cracks fall into closed rings.  Traced is the ring through the top side of the object's first pixel in row-major order.
constexpr int kContourSide = 512;                              // cs_regions_contour_max_side
constexpr int kContourWords = (kContourSide + 2 + 31) / 32;    // words of a bitmap row at the side limit: 514 bits in 17 words

struct ContourLds {
    // One bit per pixel of the box inside a border of one zero bit all round: pixel (i, j) is bit (j + 1) & 31 of word
    // (i + 1) * wpr + ((j + 1) >> 5), wpr = ceil((cols + 2) / 32) words per row.  34.1 KiB at the side limit.
    uint32_t bits[(kContourSide + 2) * kContourWords];
    int red[4];
    int walked[3];                                             // n_vertices, n_cracks, area2: thread 0 to the others
};

// pixel (i, j) of the box, -1 <= i <= rows and -1 <= j <= cols: the border reads as "not the object"
__device__ __forceinline__ bool contour_in(const uint32_t* bits, int wpr, int i, int j) {
    return (bits[(i + 1) * wpr + ((j + 1) >> 5)] >> ((j + 1) & 31)) & 1u;
}

// The ring from lattice vertex (pr, pc), heading east along the top side of the first pixel (pr, pc), by one thread.  Headings
// 0 = E, 1 = S, 2 = W, 3 = N; a step moves one crack along the heading, and at the vertex (r, c) it reaches R is the pixel ahead on
// the right and L the one ahead on the left:
//     E: R = (r, c),         L = (r - 1, c)         S: R = (r, c - 1),     L = (r, c)
//     W: R = (r - 1, c - 1), L = (r, c - 1)         N: R = (r - 1, c),     L = (r - 1, c - 1)           (L of h is R of h - 1)
// R out: turn right (with CONN 2 and L in: turn left, across to the diagonal pixel); R and L in: turn left; R in, L out: straight.
// Either way the crack that follows has a pixel of the object on its right, so every vertex reached is a corner of such a pixel,
// 0 <= r <= rows and 0 <= c <= cols, and R and L lie inside the bordered bitmap.  The walk ends on arriving at (pr, pc) with the
// new heading east; the successor rule permutes the cracks of the bitmap, so that happens after at most `bound` steps, and the
// loop stops there whatever the bitmap holds.  A vertex is written where the heading changes, (pr, pc) first.
template <int CONN>
__device__ __forceinline__ void contour_walk(const uint32_t* bits, int wpr, int pr, int pc, int bound, int r0, int c0, int maxv,
                                             int32_t* __restrict__ verts, int* walked) {
    int r = pr, c = pc, h = 0, n = 1, cracks = 0;
    int vr = pr, vc = pc;                                      // the last vertex written
    long long area2 = 0;
    if (maxv > 0) {
        verts[0] = r0 + pr;
        verts[1] = c0 + pc;
    }
    while (cracks < bound) {
        r += h == 1 ? 1 : h == 3 ? -1 : 0;
        c += h == 0 ? 1 : h == 2 ? -1 : 0;
        ++cracks;
        const int rr = r - (h >= 2), rc = c - (h == 1 || h == 2);                // R of h
        const int lr = r - (h == 0 || h == 3), lc = c - (h >= 2);                // L of h = R of h - 1
        const bool R = contour_in(bits, wpr, rr, rc), L = contour_in(bits, wpr, lr, lc);
        int nh = h;
        if (!R) nh = (CONN == 2 && L) ? (h + 3) & 3 : (h + 1) & 3;
        else if (L) nh = (h + 3) & 3;
        if (r == pr && c == pc && nh == 0) break;
        if (nh != h) {
            area2 += (long long)vc * r - (long long)c * vr;
            if (n < maxv) {
                verts[2 * n] = r0 + r;
                verts[2 * n + 1] = c0 + c;
            }
            ++n;
            vr = r;
            vc = c;
            h = nh;
        }
    }
    area2 += (long long)vc * pr - (long long)pc * vr;
    walked[0] = n;
    walked[1] = cracks;
    walked[2] = (int)area2;
}

// (-1, -1) into the vertex slots from `from` on, by the workgroup; unsigned, since 2 maxv may come close to 2^31
__device__ __forceinline__ void contour_fill(int32_t* __restrict__ verts, int from, int maxv) {
    for (unsigned k = 2u * from + threadIdx.x; k < 2u * maxv; k += 256) verts[k] = -1;
}

// One workgroup per (image, label) at a time.  The box is cut to the image before anything is read, so whatever the table holds
// no read leaves the label image; after the staging no step reads global memory or leaves the bitmap.
template <int CONN>
__global__ __launch_bounds__(256) void contour_kernel(const int32_t* __restrict__ lab, int N, int H, int W, int cap,
                                                      const int32_t* __restrict__ bbox, int maxv, int32_t* __restrict__ contour,
                                                      int32_t* __restrict__ vertices) {
    __shared__ ContourLds s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long objects = (long long)N * cap;
    for (long long q = blockIdx.x; q < objects; q += gridDim.x) {
        const int n = (int)(q / cap), l = (int)(q - (long long)n * cap) + 1;
        const int r0 = max(bbox[4 * q], 0), c0 = max(bbox[4 * q + 1], 0);
        const int rows = min(bbox[4 * q + 2], H) - r0, cols = min(bbox[4 * q + 3], W) - c0;
        int32_t* verts = vertices + 2 * q * maxv;              // never dereferenced where maxv == 0
        const bool none = rows <= 0 || cols <= 0;
        if (none || rows > kContourSide || cols > kContourSide) {      // the same in every thread: no barrier is left out below
            if (threadIdx.x < 4) contour[4 * q + threadIdx.x] = none ? 0 : -1;
            contour_fill(verts, 0, maxv);
            continue;
        }
        // 1. the bitmap: a wave per bitmap row, its lanes over 64 bitmap columns at a time; a ballot is two words of the row
        const int wpr = (cols + 2 + 31) >> 5;
        const int32_t* img = lab + (long long)n * H * W + (long long)r0 * W + c0;
        for (int i = wave; i < rows + 2; i += 4) {
            const bool inside = i >= 1 && i <= rows;
            const int32_t* row = img + (long long)(i - 1) * W;        // read where `inside` only
            for (int j0 = 0; j0 < cols + 2; j0 += 64) {
                const int j = j0 + lane - 1;                           // the box column of bitmap column j0 + lane
                const unsigned long long bal = __ballot(inside && j >= 0 && j < cols && row[j] == l);
                const int w = (j0 >> 5) + lane;
                if (lane < 2 && w < wpr) s.bits[i * wpr + w] = (uint32_t)(bal >> (32 * lane));
            }
        }
        __syncthreads();
        // 2. all boundary cracks of the label, a word of 32 pixels at a time, and its first pixel in row-major order
        int cracks_all = 0, first = INT_MAX;
        for (int k = threadIdx.x; k < rows * wpr; k += 256) {
            const int i = k / wpr + 1, w = k - (i - 1) * wpr;
            const uint32_t* p = s.bits + i * wpr + w;
            const uint32_t x = *p;
            if (x == 0) continue;
            const uint32_t west = x << 1 | (w > 0 ? p[-1] >> 31 : 0u), east = x >> 1 | (w + 1 < wpr ? p[1] << 31 : 0u);
            cracks_all += __popc(x & ~p[-wpr]) + __popc(x & ~p[wpr]) + __popc(x & ~west) + __popc(x & ~east);
            first = min(first, (k << 5) + __ffs(x) - 1);
        }
        cracks_all = block_reduce<256>(cracks_all, [](int x, int y) { return x + y; }, s.red);
        first = block_reduce<256>(first, [](int x, int y) { return min(x, y); }, s.red);
        if (first == INT_MAX) {                                        // the same in every thread; the bitmap is free again
            if (threadIdx.x < 4) contour[4 * q + threadIdx.x] = 0;
            contour_fill(verts, 0, maxv);
            continue;
        }
        // 3. the walk, by one thread; the others wait for the vertex count
        if (threadIdx.x == 0) {
            const int k = first >> 5;
            const int pr = k / wpr, pc = ((k - pr * wpr) << 5) + (first & 31) - 1;
            contour_walk<CONN>(s.bits, wpr, pr, pc, 2 * rows * cols + rows + cols, r0, c0, maxv, verts, s.walked);
        }
        __syncthreads();
        // (thread 0 writes `walked` again only behind the next object's barriers, which every thread reaches after this read)
        const int nv = s.walked[0];
        if (threadIdx.x < 3) contour[4 * q + threadIdx.x] = s.walked[threadIdx.x];
        if (threadIdx.x == 3) contour[4 * q + 3] = cracks_all;
        contour_fill(verts, min(nv, maxv), maxv);
    }
}

// ---- how a stain is arranged inside every label: grey-level co-occurrence per direction, folded to Haralick's tables --------------
// A pixel's level is the byte of a plane, or the level of one stain of an RGB pixel by quantify's rule with ONE row of Mq per
// image; its grey level is g = level * L >> 8, L in {8, 16, 32}.  Direction k = 0 .. 3 has the offset (0, d), (d, d), (d, 0),
// (d, -d).  A pixel p of label l pairs with q = p + offset where q lies inside the image and has the label l too: C_k[g(p)][g(q)]
// += 1.  S_k = C_k + C_k^T; written per (image, row, direction) are the pair count, diff[x] = sum over |i - j| = x of S_ij,
// sum[x] = the same over i + j = x, marg[i] = sum over j of S_ij, sq = sum of S_ij^2, cross = sum of i j S_ij and, where asked
// for, S itself.  With H W <= 2^30 a direction has fewer than 2^30 pairs: every S_ij < 2^31, sq < 2^62, cross < 2^41.
constexpr int kTexLevels = 32;                                 // the largest L: four tables of 32 x 32 counters are 16 KiB

enum TextureSrc { kTexPlane, kTexRgb };

struct TextureTables {
    int32_t* pairs;      // [N][cap][4]
    int32_t* diff;       // [N][cap][4][L]
    int32_t* sum;        // [N][cap][4][2L - 1]
    int32_t* marg;       // [N][cap][4][L]
    long long* sq;       // [N][cap][4]
    long long* cross;    // [N][cap][4]
    int32_t* matrix;     // [N][cap][4][L][L] or NULL
};

struct TextureLds {
    // C_k as [k][i][j] with the row length L of the call, and the three histograms laid out as a row of their output tables
    uint32_t c[4 * kTexLevels * kTexLevels];
    uint32_t diff[4 * kTexLevels], sum[4 * (2 * kTexLevels - 1)], marg[4 * kTexLevels], pairs[4];
    long long red[4];
    int32_t od[256];                                           // od_q, read on the RGB route only
};

// One workgroup per (image, label) at a time.  The box is cut to the image before anything is read and every partner is held
// against the image's own sides, so whatever the table holds no read leaves the label image or the source.  A wave walks a row of
// the box with its lanes along the columns; every add to LDS is one that returns nothing.  After the walk the workgroup folds its
// four tables and writes its own output row with plain stores, zeros included: nothing is zeroed beforehand, nothing is added to
// global memory, and the result does not depend on launch or arrival order.
template <TextureSrc SRC>
__global__ __launch_bounds__(256) void texture_kernel(const int32_t* __restrict__ lab, const uint8_t* __restrict__ src, int N, int H, int W,
                                                      const int32_t* __restrict__ od_q, const int32_t* __restrict__ Mq, int cap,
                                                      const int32_t* __restrict__ bbox, int L, int d, TextureTables t) {
    __shared__ TextureLds s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int LL = L * L, S2 = 2 * L - 1, shift = L == 8 ? 3 : L == 16 ? 4 : 5;
    if (SRC == kTexRgb) s.od[tid] = od_q[tid];                  // (the first barrier of the first object publishes it)
    const long long objects = (long long)N * cap;
    for (long long q = blockIdx.x; q < objects; q += gridDim.x) {
        const int n = (int)(q / cap), l = (int)(q - (long long)n * cap) + 1;
        const int r0 = max(bbox[4 * q], 0), c0 = max(bbox[4 * q + 1], 0), r1 = min(bbox[4 * q + 2], H), c1 = min(bbox[4 * q + 3], W);
        const bool none = r1 <= r0 || c1 <= c0;                        // the same in every thread: no barrier is left out below
        for (int i = tid; i < 4 * LL; i += 256) {
            s.c[i] = 0;
            if (none && t.matrix) t.matrix[q * 4 * LL + i] = 0;
        }
        for (int i = tid; i < 4 * S2; i += 256) {
            s.sum[i] = 0;
            if (i < 4 * L) s.diff[i] = s.marg[i] = 0;
            if (i < 4) s.pairs[i] = 0;
        }
        __syncthreads();
        if (!none) {
            // 1. the ordered counts: a wave per row of the box, every pixel of the label looks at its four partners
            const long long base = (long long)n * H * W;
            long long m0 = 0, m1 = 0, m2 = 0;
            if (SRC == kTexRgb) m0 = Mq[3 * n], m1 = Mq[3 * n + 1], m2 = Mq[3 * n + 2];
            auto grey = [&](long long p) {
                if (SRC == kTexPlane) return (int)src[p] * L >> 8;
                const uint8_t* px = src + 3 * p;
                const long long sh = (m0 * s.od[px[0]] + m1 * s.od[px[1]] + m2 * s.od[px[2]] + (1LL << 23)) >> 24;
                return (int)(sh < 0 ? 0 : sh > 255 ? 255 : sh) * L >> 8;
            };
            for (int r = r0 + wave; r < r1; r += 4) {
                const long long row = base + (long long)r * W;
                for (int c = c0 + lane; c < c1; c += 64) {
                    if (lab[row + c] != l) continue;
                    const int gp = grey(row + c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int rr = r + (k == 0 ? 0 : d), cc = c + (k < 2 ? d : k == 2 ? 0 : -d);
                        if (rr >= H || cc < 0 || cc >= W) continue;
                        const long long pq = base + (long long)rr * W + cc;
                        if (lab[pq] != l) continue;
                        __hip_atomic_fetch_add(s.c + k * LL + (gp << shift) + grey(pq), 1u, __ATOMIC_RELAXED, kLds);
                    }
                }
            }
            __syncthreads();
            // 2. S = C + C^T of every direction, folded into the histograms (adds to LDS) and the two sums (block_reduce)
            for (int k = 0; k < 4; ++k) {
                const uint32_t* ck = s.c + k * LL;
                long long sq = 0, cross = 0;
                for (int e = tid; e < LL; e += 256) {
                    const int i = e >> shift, j = e & (L - 1);
                    const uint32_t cij = ck[e], sij = cij + ck[j * L + i];
                    if (t.matrix) t.matrix[(q * 4 + k) * LL + e] = (int32_t)sij;
                    if (sij == 0) continue;
                    __hip_atomic_fetch_add(s.diff + k * L + abs(i - j), sij, __ATOMIC_RELAXED, kLds);
                    __hip_atomic_fetch_add(s.sum + k * S2 + i + j, sij, __ATOMIC_RELAXED, kLds);
                    __hip_atomic_fetch_add(s.marg + k * L + i, sij, __ATOMIC_RELAXED, kLds);
                    if (cij) __hip_atomic_fetch_add(s.pairs + k, cij, __ATOMIC_RELAXED, kLds);
                    sq += (long long)sij * sij;
                    cross += (long long)(i * j) * sij;
                }
                sq = block_reduce<256>(sq, [](long long x, long long y) { return x + y; }, s.red);
                cross = block_reduce<256>(cross, [](long long x, long long y) { return x + y; }, s.red);
                if (tid == 0) {
                    t.sq[q * 4 + k] = sq;
                    t.cross[q * 4 + k] = cross;
                }
            }
            // (the last barrier of block_reduce is behind every add above)
        } else if (tid < 4) {
            t.sq[q * 4 + tid] = 0;
            t.cross[q * 4 + tid] = 0;
        }
        // 3. the row of this label: the histograms as they lie in LDS
        for (int i = tid; i < 4 * S2; i += 256) {
            t.sum[q * 4 * S2 + i] = (int32_t)s.sum[i];
            if (i < 4 * L) {
                t.diff[q * 4 * L + i] = (int32_t)s.diff[i];
                t.marg[q * 4 * L + i] = (int32_t)s.marg[i];
            }
            if (i < 4) t.pairs[q * 4 + i] = (int32_t)s.pairs[i];
        }
        __syncthreads();                                               // the next object zeroes the tables
    }
}

// ---- two label images walked at once: what match and overlap share ---------------------------------------------------------------
struct PairSides {
    int32_t *area_pred, *area_truth;   // [N][cap_pred], [N][cap_truth]
    int32_t *maxp, *maxt;              // [N] or NULL: the largest pred / truth label
    int cap_pred, cap_truth;
};

// element i of an init launch over at least max(N cap_pred, N cap_truth) >= N elements
__device__ __forceinline__ void pair_sides_init(const PairSides& s, int N, long long i) {
    if (i < (long long)N * s.cap_pred) s.area_pred[i] = 0;
    if (i < (long long)N * s.cap_truth) s.area_truth[i] = 0;
    if (i < N && s.maxp) s.maxp[i] = 0;
    if (i < N && s.maxt) s.maxt[i] = 0;
}

// A run is a stretch of a wave's lanes on which both labels are constant and at least one is positive (0 and below = background);
// it starts where either label differs from the left neighbour's.  head: this lane acts for the whole run of len lanes with pred
// label p and truth label g, both clamped: a label above its side's capacity is background.  ACCOUNT: a head lane first raises
// image n's maxima to its labels as they are, and after the clamp adds the run to the areas.  Called by the whole wave.
struct PairRun { bool head; int len, p, g; };
template <bool ACCOUNT>
__device__ __forceinline__ PairRun pair_run(const int32_t* __restrict__ pred, const int32_t* __restrict__ truth, const PairSides& s, int n,
                                            int W, int c, long long px) {
    PairRun u{false, 1, c < W ? max(pred[px], 0) : 0, c < W ? max(truth[px], 0) : 0};
    const bool live = (u.p | u.g) != 0;
    const unsigned long long bal = __ballot(live);
    if (bal == 0) return u;
    const int pl = __shfl_up(u.p, 1), gl = __shfl_up(u.g, 1);          // (lane 0 gets its own back)
    u.head = run_of(bal, __ballot(live && (u.p != pl || u.g != gl)), threadIdx.x & 63, u.len);
    if (!u.head) return u;
    if (ACCOUNT && s.maxp && u.p) raise_to(s.maxp + n, u.p);
    if (ACCOUNT && s.maxt && u.g) raise_to(s.maxt + n, u.g);
    u.p = u.p <= s.cap_pred ? u.p : 0;
    u.g = u.g <= s.cap_truth ? u.g : 0;
    if (ACCOUNT && u.g) __hip_atomic_fetch_add(s.area_truth + (long long)n * s.cap_truth + u.g - 1, u.len, __ATOMIC_RELAXED, kGlobal);
    if (ACCOUNT && u.p) __hip_atomic_fetch_add(s.area_pred + (long long)n * s.cap_pred + u.p - 1, u.len, __ATOMIC_RELAXED, kGlobal);
    return u;
}

// ---- label image against label image: object matches at IoU > 1/2 -----------------------------------------------------------------
// pred label p and truth label g match iff 2 I(p, g) > Ap + At - I.  Such a g covers more than half of p's pixels, so bit b of g is
// set exactly where more than half of p's pixels carry a truth label with bit b set: B = bit_length(cap_truth) counters per pred
// label spell the only possible partner, one more pass counts its intersection, and the test itself is made on exact integers.
struct Match {
    PairSides s;
    int32_t* match;        // [N][cap_pred]   the truth label matched, 0 = none
    int32_t* inter;        // [N][cap_pred]   I(p, match)
    int32_t* match_truth;  // [N][cap_truth]  the pred label matched, 0 = none
    int32_t* vote;         // [N][cap_pred][B]
    int32_t* cand;         // [N][cap_pred]
    int B;
};

__global__ __launch_bounds__(256) void match_init_kernel(int N, Match t) {
    const long long np = (long long)N * t.s.cap_pred, nt = (long long)N * t.s.cap_truth, nv = np * t.B;
    const long long all = nv > nt ? nv : nt;                           // >= np >= N
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long long)gridDim.x * 256) {
        pair_sides_init(t.s, N, i);
        if (i < nv) t.vote[i] = 0;
        if (i < np) t.inter[i] = 0;
        if (i < nt) t.match_truth[i] = 0;
    }
}

// VOTE: the accounting of both sides and, for every set bit b of the truth label, vote[p][b] += len.  Otherwise: inter[p] += len
// on the runs whose truth label is p's candidate.
template <bool VOTE>
__global__ __launch_bounds__(256) void match_walk_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ truth, int N, int H,
                                                         int W, Match t) {
    walk_row_segments(N, H, W, [&](int n, int, int c, long long px) {
        const PairRun u = pair_run<VOTE>(pred, truth, t.s, n, W, c, px);
        if (!u.head || !u.p) return;
        const long long q = (long long)n * t.s.cap_pred + u.p - 1;     // p's row
        if (VOTE) {
            for (unsigned bits = (unsigned)u.g; bits; bits &= bits - 1)   // g <= cap_truth < 2^B: every set bit is below B
                __hip_atomic_fetch_add(t.vote + q * t.B + __builtin_ctz(bits), u.len, __ATOMIC_RELAXED, kGlobal);
        } else if (u.g && t.cand[q] == u.g) {
            __hip_atomic_fetch_add(t.inter + q, u.len, __ATOMIC_RELAXED, kGlobal);
        }
    });
}

// One thread per pred label: the truth label spelled by the bits that more than half of the label's pixels voted for.  Without a
// majority partner the votes can spell any number, one above cap_truth included: that is no candidate.
__global__ __launch_bounds__(256) void match_candidate_kernel(long long rows, Match t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const long long area = t.s.area_pred[i];
        int g = 0;
        for (int b = 0; b < t.B; ++b)
            if (2 * (long long)t.vote[i * t.B + b] > area) g |= 1 << b;
        t.cand[i] = g <= t.s.cap_truth ? g : 0;
    }
}

// One thread per pred label: the test itself, in 64-bit integers.  A truth label is matched by at most one pred label (two would
// each hold more than half of its pixels), so the stores into match_truth never meet.
__global__ __launch_bounds__(256) void match_decide_kernel(long long rows, Match t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const int g = t.cand[i];
        const long long n = i / t.s.cap_pred;
        const long long in = t.inter[i];
        bool ok = false;
        if (g > 0) {
            const long long uni = (long long)t.s.area_pred[i] + (long long)t.s.area_truth[n * t.s.cap_truth + g - 1] - in;
            ok = 2 * in > uni;
        }
        t.match[i] = ok ? g : 0;
        if (ok)
            t.match_truth[n * t.s.cap_truth + g - 1] = (int)(i - n * t.s.cap_pred) + 1;
        else
            t.inter[i] = 0;
    }
}

// ---- a sparse table of label pairs: what overlap and adjacency share --------------------------------------------------------------
// Per image an open-addressing hash table of `slots` (a power of two) 64-bit keys, (hi << 32) | lo, 0 = empty, and one or more
// arrays of as many int32 counts, which the owner of the table holds.  A key is written once, by the CAS that takes the slot from
// empty, and never changes: a probe that reads a key other than 0 has read the slot's final key.  Which slot a pair lands in depends
// on the order of arrival; the set of (key, counts) does not (integer sums).
struct PairTable {
    int32_t* n_pairs;               // [N]  occupied slots
    int32_t* dropped;               // [N]  runs that found no slot
    unsigned long long* keys;       // [N][slots]
    int slots;
};

// element i of an init launch over at least N slots >= N elements (the count arrays are their owner's to clear)
__device__ __forceinline__ void pair_table_init(const PairTable& p, int N, long long i) {
    if (i < (long long)N * p.slots) p.keys[i] = 0;
    if (i < N) {
        p.n_pairs[i] = 0;
        p.dropped[i] = 0;
    }
}

__device__ __forceinline__ unsigned pair_hash(unsigned p, unsigned g) {
    unsigned h = p * 0x9E3779B1u ^ g * 0x85EBCA77u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    return h ^ (h >> 13);
}

// len more for pair (p, g) of one image's table.  At most `slots` probes: a slot is taken from empty by CAS, one that
// holds this key (from this CAS or from another thread's) gets the add, any other key sends the probe on.  Nothing is waited for.
// Returns false when every slot holds another key.  *fresh: this call took a slot.
__device__ __forceinline__ bool pair_insert(unsigned long long* keys, int32_t* cnt, unsigned mask, int p, int g, int len, bool* fresh) {
    const unsigned long long key = ((unsigned long long)(unsigned)p << 32) | (unsigned)g;
    unsigned s = pair_hash((unsigned)p, (unsigned)g) & mask;
    *fresh = false;
    for (unsigned tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
        unsigned long long seen = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, kGlobal);
        if (seen == 0) {                                               // (on failure the CAS leaves the key it met in `seen`)
            if (__hip_atomic_compare_exchange_strong(keys + s, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kGlobal)) {
                *fresh = true;
                seen = key;
            }
        }
        if (seen == key) {
            __hip_atomic_fetch_add(cnt + s, len, __ATOMIC_RELAXED, kGlobal);
            return true;
        }
    }
    return false;
}

// A run of len for pair (p, g) of image n into the count array cnt [N][slots] of the table: a run that finds no slot is counted in
// dropped[n], one that takes a slot in n_pairs[n].  `p` must be a copy of the table in a local of the kernel: with the two counters
// read through the kernel's argument inside a walker's body, the compiler merges the two adds below into one whose pointer it picks
// from the argument by a run-time index, and that keeps a copy of those 16 bytes of it in scratch (24 bytes, hipcc of ROCm 7).
__device__ __forceinline__ void pair_add(const PairTable& p, int32_t* cnt, int n, int hi, int lo, int len) {
    const long long base = (long long)n * p.slots;                     // < N slots < 2^31
    bool fresh;
    if (!pair_insert(p.keys + base, cnt + base, (unsigned)p.slots - 1, hi, lo, len, &fresh))
        __hip_atomic_fetch_add(p.dropped + n, 1, __ATOMIC_RELAXED, kGlobal);
    else if (fresh)
        __hip_atomic_fetch_add(p.n_pairs + n, 1, __ATOMIC_RELAXED, kGlobal);
}

// ---- label image against label image: every overlapping pair ----------------------------------------------------------------------
// The sparse contingency table of two label images: every (p, g) that shares a pixel, with the count, in a PairTable with key
// (p << 32) | g and one count array.  Everything derived from the table is a maximum under a total order of the pairs, which does
// not depend on where they sit.
struct Overlap {
    PairSides s;
    PairTable pairs;
    int32_t* iou_partner;           // [N][cap_truth]  the pred label of largest IoU, 0 = none
    int32_t* iou_inter;             // [N][cap_truth]  its intersection
    int32_t* inter_partner_truth;   // [N][cap_truth]  the pred label of largest intersection
    int32_t* inter_truth;           // [N][cap_truth]
    int32_t* inter_partner_pred;    // [N][cap_pred]   the truth label of largest intersection
    int32_t* inter_pred;            // [N][cap_pred]
    int32_t* cnt;                   // [N][slots]
    unsigned long long* best_iou;   // [N][cap_truth]  (I << 32) | p, 0 = none
    unsigned long long* best_it;    // [N][cap_truth]  (I << 32) | ~p: the largest I, then the lowest p
    unsigned long long* best_ip;    // [N][cap_pred]   (I << 32) | ~g
};

__global__ __launch_bounds__(256) void overlap_init_kernel(int N, Overlap t) {
    const long long np = (long long)N * t.s.cap_pred, nt = (long long)N * t.s.cap_truth, ns = (long long)N * t.pairs.slots;
    const long long all = max(ns, max(np, nt));                        // >= N
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long long)gridDim.x * 256) {
        pair_sides_init(t.s, N, i);
        pair_table_init(t.pairs, N, i);
        if (i < ns) t.cnt[i] = 0;
        if (i < np) t.best_ip[i] = 0;
        if (i < nt) {
            t.best_iou[i] = 0;
            t.best_it[i] = 0;
        }
    }
}

// The accounting of both sides, and every run on which both labels are positive (and within their capacities) adds its length to
// its pair's slot.
__global__ __launch_bounds__(256) void overlap_walk_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ truth, int N, int H,
                                                           int W, Overlap t) {
    const PairTable pairs = t.pairs;                                   // (a local: see pair_add)
    walk_row_segments(N, H, W, [&](int n, int, int c, long long px) {
        const PairRun u = pair_run<true>(pred, truth, t.s, n, W, c, px);
        if (u.head && u.p && u.g) pair_add(pairs, t.cnt, n, u.p, u.g, u.len);
    });
}

// One thread per slot, after the walk: the areas and counts are final.  Best intersection of either side: an atomic maximum of
// (I << 32) | ~partner, i.e. the largest I and among equals the lowest partner.  Best IoU of a truth label: I / U > I' / U' is
// I U' > I' U in 64-bit integers (all four below 2^31), equal quotients go to the lower pred label; the holder is replaced by
// CAS only where this slot's pair is strictly better under that total order, so a failed CAS means that another thread improved
// the holder, the comparison is made again against what it wrote, and the loop ends with the best pair of all whatever the order.
__global__ __launch_bounds__(256) void overlap_reduce_kernel(long long n_slots, Overlap t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (long long)gridDim.x * 256) {
        const unsigned long long key = t.pairs.keys[i];
        if (key == 0) continue;
        const long long n = i / t.pairs.slots;
        const unsigned p = (unsigned)(key >> 32), g = (unsigned)key;
        const unsigned long long I = (unsigned)t.cnt[i];
        const long long qp = n * t.s.cap_pred + p - 1, qg = n * t.s.cap_truth + g - 1;
        __hip_atomic_fetch_max(t.best_it + qg, (I << 32) | (unsigned)~p, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_max(t.best_ip + qp, (I << 32) | (unsigned)~g, __ATOMIC_RELAXED, kGlobal);
        const long long at = t.s.area_truth[qg];
        const unsigned long long U = (unsigned long long)(t.s.area_pred[qp] + at - (long long)I);
        const unsigned long long mine = (I << 32) | p;
        unsigned long long held = __hip_atomic_load(t.best_iou + qg, __ATOMIC_RELAXED, kGlobal);
        for (;;) {
            if (held != 0) {
                const unsigned hp = (unsigned)held;
                const unsigned long long hI = held >> 32;
                const unsigned long long hU = (unsigned long long)(t.s.area_pred[n * t.s.cap_pred + hp - 1] + at - (long long)hI);
                const unsigned long long a = I * hU, b = hI * U;
                if (!(a > b || (a == b && p < hp))) break;             // the holder is as good or better
            }
            if (__hip_atomic_compare_exchange_strong(t.best_iou + qg, &held, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kGlobal)) break;
        }
    }
}

// One thread per label of either side: the packed winners into the tables.
__global__ __launch_bounds__(256) void overlap_finish_kernel(int N, Overlap t) {
    const long long np = (long long)N * t.s.cap_pred, nt = (long long)N * t.s.cap_truth;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < max(np, nt); i += (long long)gridDim.x * 256) {
        if (i < nt) {
            const unsigned long long q = t.best_iou[i], b = t.best_it[i];
            t.iou_partner[i] = (int)(unsigned)q;
            t.iou_inter[i] = (int)(q >> 32);
            t.inter_partner_truth[i] = b ? (int)~(unsigned)b : 0;
            t.inter_truth[i] = (int)(b >> 32);
        }
        if (i < np) {
            const unsigned long long b = t.best_ip[i];
            t.inter_partner_pred[i] = b ? (int)~(unsigned)b : 0;
            t.inter_pred[i] = (int)(b >> 32);
        }
    }
}

// ---- one label image against its own shifted self: which labels touch which -------------------------------------------------------
// A pixel's id is its label where 1 <= label <= cap, else 0.  An interior side is an unordered pair of 4-adjacent pixels, an
// exterior side a pixel side on the image edge.  sides(a, b), a < b both positive: the interior sides with ids {a, b}; corners(a, b)
// (CONN 2 only): the diagonal pixel pairs {(r, c), (r + 1, c + 1)} and {(r, c + 1), (r + 1, c)} with ids {a, b}.  The pairs live in
// a PairTable, key (a << 32) | b, with two count arrays; a slot exists iff one of its two counts is positive.  Per label:
// background = interior sides with ids {a, 0}, outside = exterior sides of a's pixels, contact = the sum of sides over a's pairs,
// n_neighbors = a's pairs, partner = the pair of largest sides, ties to the lower label.
struct Adjacency {
    int32_t* maxlab;                // [N] or NULL: the largest label, also above cap
    PairTable pairs;
    int32_t* n_neighbors;           // [N][cap]
    int32_t* contact;               // [N][cap]
    int32_t* background;            // [N][cap]
    int32_t* outside;               // [N][cap]
    int32_t* partner;               // [N][cap]
    int32_t* partner_sides;         // [N][cap]
    int32_t* sides;                 // [N][slots]
    int32_t* corners;               // [N][slots]
    unsigned long long* best;       // [N][cap]  (sides << 32) | ~partner, 0 = no neighbour
    int cap;
};

__global__ __launch_bounds__(256) void adjacency_init_kernel(int N, Adjacency t) {
    const long long nl = (long long)N * t.cap, ns = (long long)N * t.pairs.slots;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < max(nl, ns); i += (long long)gridDim.x * 256) {
        pair_table_init(t.pairs, N, i);                                // (N <= ns)
        if (i < ns) {
            t.sides[i] = 0;
            t.corners[i] = 0;
        }
        if (i < nl) {
            t.n_neighbors[i] = 0;
            t.contact[i] = 0;
            t.background[i] = 0;
            t.outside[i] = 0;
            t.best[i] = 0;
        }
        if (i < N && t.maxlab) t.maxlab[i] = 0;                        // N <= nl
    }
}

// A wave holds its 64 columns of rows r - 1, r, r + 1 (edge_kernel's access pattern).  Every interior side and every diagonal pair
// is counted by exactly one pixel: the left one of a horizontal side, the upper one of a vertical side, and pixel (r, c) for the two
// diagonals of the 2 x 2 block whose top left corner it is.  What a row adds to a pair goes out per run of lanes on which the two
// ids are constant, one insert with the run's length; the background / outside tallies of a pixel are summed over the runs of
// constant id and added once per run.
template <int CONN>
__global__ __launch_bounds__(256) void adjacency_walk_kernel(const int32_t* __restrict__ lab, int N, int H, int W, Adjacency t) {
    const int lane = threadIdx.x & 63;
    const int cap = t.cap;
    const PairTable pairs = t.pairs;                                   // (a local: see pair_add)
    auto id_of = [cap](int l) { return (l >= 1 && l <= cap) ? l : 0; };
    walk_row_segments(N, H, W, [&](int n, int r, int c, long long p) {
        const bool in = c < W, above = r > 0, below = r < H - 1;
        const int raw = in ? lab[p] : 0;
        const int m = id_of(raw);
        const int u = (in && above) ? id_of(lab[p - W]) : 0, d = (in && below) ? id_of(lab[p + W]) : 0;
        const int raw_left = __shfl_up(raw, 1);                        // (lane 0 gets its own back)
        if (t.maxlab && raw > 0 && (lane == 0 || raw != raw_left)) raise_to(t.maxlab + n, raw);
        int left = __shfl_up(m, 1), right = __shfl_down(m, 1), dr = __shfl_down(d, 1);   // a lane with c >= W carries 0
        if (lane == 0) left = c > 0 ? id_of(lab[p - 1]) : 0;
        if (lane == 63) {
            const bool has = c + 1 < W;
            right = has ? id_of(lab[p + 1]) : 0;
            dr = (has && below) ? id_of(lab[p + W + 1]) : 0;
        }
        if (__ballot((m | right) != 0) == 0) return;                    // every side and corner counted here has m or right in it
        const bool has_right = c + 1 < W;                              // (then c < W too)

        int tally = 0;                                                 // outside | background << 16, at most 4 each per pixel
        if (m > 0) {
            tally = (int)!above + (int)!below + (int)(c == 0) + (int)!has_right;
            tally += ((int)(c > 0 && left == 0) + (int)(has_right && right == 0) + (int)(above && u == 0) + (int)(below && d == 0)) << 16;
        }
        const int m_left = __shfl_up(m, 1);
        int len;
        const bool head = run_of(__ballot(m > 0), __ballot(m > 0 && m != m_left), lane, len);
        tally = run_sum(tally, lane, m > 0 ? lane + len - 1 : lane);
        if (head) {
            const long long q = (long long)n * cap + m - 1;
            if (tally & 0xFFFF) __hip_atomic_fetch_add(t.outside + q, tally & 0xFFFF, __ATOMIC_RELAXED, kGlobal);
            if (tally >> 16) __hip_atomic_fetch_add(t.background + q, tally >> 16, __ATOMIC_RELAXED, kGlobal);
        }

        // the runs of constant (a, b) among the lanes where `ok` and the two ids are positive and differ: one insert each
        auto emit = [&](int a, int b, bool ok, int32_t* cnt) {
            const bool live = ok && a > 0 && b > 0 && a != b;
            const unsigned long long bal = __ballot(live);
            if (bal == 0) return;
            const int al = __shfl_up(a, 1), bl = __shfl_up(b, 1);
            int n_run;
            if (run_of(bal, __ballot(live && (a != al || b != bl)), lane, n_run)) pair_add(pairs, cnt, n, min(a, b), max(a, b), n_run);
        };
        emit(m, d, below, t.sides);                                    // (d is 0 where c >= W)
        emit(m, right, has_right, t.sides);
        if (CONN == 2) {
            emit(m, dr, has_right && below, t.corners);
            emit(right, d, has_right && below, t.corners);
        }
    });
}

// One thread per slot, after the walk: both labels of the pair get a neighbour, its sides, and the atomic maximum of
// (sides << 32) | ~other, i.e. the largest sides and among equals the lowest label.
__global__ __launch_bounds__(256) void adjacency_reduce_kernel(long long n_slots, Adjacency t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (long long)gridDim.x * 256) {
        const unsigned long long key = t.pairs.keys[i];
        if (key == 0) continue;
        const long long n = i / t.pairs.slots;
        const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
        const int s = t.sides[i];
        const long long qa = n * t.cap + a - 1, qb = n * t.cap + b - 1;
        __hip_atomic_fetch_add(t.n_neighbors + qa, 1, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_add(t.n_neighbors + qb, 1, __ATOMIC_RELAXED, kGlobal);
        if (s) {
            __hip_atomic_fetch_add(t.contact + qa, s, __ATOMIC_RELAXED, kGlobal);
            __hip_atomic_fetch_add(t.contact + qb, s, __ATOMIC_RELAXED, kGlobal);
        }
        const unsigned long long hi = (unsigned long long)(unsigned)s << 32;
        __hip_atomic_fetch_max(t.best + qa, hi | (unsigned)~b, __ATOMIC_RELAXED, kGlobal);
        __hip_atomic_fetch_max(t.best + qb, hi | (unsigned)~a, __ATOMIC_RELAXED, kGlobal);
    }
}

// One thread per label: the packed winner into the tables.
__global__ __launch_bounds__(256) void adjacency_finish_kernel(long long rows, Adjacency t) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const unsigned long long b = t.best[i];
        t.partner[i] = b ? (int)~(unsigned)b : 0;
        t.partner_sides[i] = (int)(b >> 32);
    }
}

// ---- the seed label image of a point set: 0 everywhere, k + 1 at the pixel of live point k, the lowest k of a pixel -------------
// A point is live when it is within its image's limit and inside the image.  CLAIM: the pixel is raised to ~k as an unsigned
// number (the largest for the lowest k, never 0).  Otherwise, in a later launch: the point whose ~k the pixel holds writes k + 1.
// k + 1 is never another point's ~k' (k + k' + 1 < 2^32 - 1), so whichever order the writes land in, only the owner writes.
template <bool CLAIM>
__global__ __launch_bounds__(256) void seed_labels_kernel(PointSet s, int N, int H, int W, int32_t* __restrict__ out) {
    const long long HW = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < s.P; p += (long long)gridDim.x * 256) {
        const int n = point_image(s, N, p);
        if (n < 0) continue;
        const PointWindow w = point_window(s, n);
        const long long k = p - w.o0;
        if (k >= w.kept) continue;
        const long long r = s.pts[2 * p], c = s.pts[2 * p + 1];
        if (r < 0 || r >= H || c < 0 || c >= W) continue;
        unsigned* at = reinterpret_cast<unsigned*>(out) + (n * HW + r * W + c);
        const unsigned mine = ~(unsigned)k;
        if (CLAIM)
            __hip_atomic_fetch_max(at, mine, __ATOMIC_RELAXED, kGlobal);
        else if (__hip_atomic_load(at, __ATOMIC_RELAXED, kGlobal) == mine)
            __hip_atomic_store(at, (unsigned)k + 1u, __ATOMIC_RELAXED, kGlobal);
    }
}

__global__ __launch_bounds__(256) void zero_labels_kernel(long long total, int32_t* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) out[i] = 0;
}

// ---- label image against label image: squared Hausdorff distance of every object to its partner ----------------------------------
// d2(A -> B) = max over ALL pixels a of A of min over the pixels b of B of dr^2 + dc^2; H2 = max of the two directions.  A job is a
// pair (object, partner or candidate) and one workgroup computes both of its directions.  For A -> B the workgroup walks B's
// bounding box and stages B's horizontal runs (row, first column, last column) in LDS, kHausStage at a time; the threads share out
// the pixels of A's bounding box, kHausPix each at a time, and every pixel of A takes the minimum over the staged runs of
// dr^2 + max(c0 - c, 0, c - c1)^2 -- all lanes read the same run, an LDS broadcast.  A target with more runs than the stage is
// staged in chunks, the minima staying in registers; a source with more pixels than one turn takes the target again per turn
// (not when the target fits the stage: it then stays).  An object without a partner is held against every object of the other side
// whose box does not rule it out.  Rows are numbered truth first: row = n cap_truth + g - 1, then
// N cap_truth + n cap_pred + p - 1.  An object is a label whose bounding box the walk of THIS call filled, so every box read lies
// inside the image whatever the partner tables hold.
constexpr int kHausStage = 2048;       // runs per stage: 16 KiB of LDS
constexpr int kHausPix = 4;            // pixels of the source per thread and turn

struct Haus {
    const int32_t *pred, *truth;
    const int32_t *given_truth, *given_pred;   // [N][cap_truth], [N][cap_pred]: the best-intersection partner, 0 = none
    int32_t *partner_truth, *d2_truth;         // [N][cap_truth]
    int32_t *partner_pred, *d2_pred;           // [N][cap_pred]
    int32_t *box_truth, *box_pred;             // [N][cap][4] = r0, c0, r1, c1 (half-open); r1 = 0: no object
    unsigned long long* best;                  // [rows]  (H2 << 32) | candidate label, all ones = none
    int32_t* list;                             // [rows]  the rows of the objects without a given partner, in no particular order
    int32_t* bound;                            // [rows]  of a listed row: an upper bound of its smallest H2, from the boxes alone
    int32_t* n_list;                           // [1]
    int N, H, W, cap_pred, cap_truth;
};

struct HausSide {                              // one side of a job: the image, the label and its box
    const int32_t* img;
    int label, r0, c0, r1, c1;
};

__global__ __launch_bounds__(256) void hausdorff_init_kernel(Haus t) {
    const long long nt = (long long)t.N * t.cap_truth, np = (long long)t.N * t.cap_pred;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nt + np; i += (long long)gridDim.x * 256) {
        int32_t* box = i < nt ? t.box_truth + 4 * i : t.box_pred + 4 * (i - nt);
        box[0] = INT_MAX;
        box[1] = INT_MAX;
        box[2] = 0;
        box[3] = 0;
        t.best[i] = ~0ull;
        t.bound[i] = INT_MAX;
        if (i == 0) *t.n_list = 0;
    }
}

// the bounding box of every label of both images (labels above the side's capacity are background)
__global__ __launch_bounds__(256) void hausdorff_box_kernel(Haus t) {
    const PairSides s{nullptr, nullptr, nullptr, nullptr, t.cap_pred, t.cap_truth};
    walk_row_segments(t.N, t.H, t.W, [&](int n, int r, int c, long long px) {
        const PairRun u = pair_run<false>(t.pred, t.truth, s, n, t.W, c, px);
        if (!u.head) return;
        if (u.g) {
            int32_t* box = t.box_truth + 4 * ((long long)n * t.cap_truth + u.g - 1);
            lower_to(box, r);
            lower_to(box + 1, c);
            raise_to(box + 2, r + 1);
            raise_to(box + 3, c + u.len);
        }
        if (u.p) {
            int32_t* box = t.box_pred + 4 * ((long long)n * t.cap_pred + u.p - 1);
            lower_to(box, r);
            lower_to(box + 1, c);
            raise_to(box + 2, r + 1);
            raise_to(box + 3, c + u.len);
        }
    });
}

struct HausLds {
    int2 run[kHausStage];              // (row, first column | last column << 16): columns are below 2^16 where d2 fits int32
    int heads[2][4];                   // the runs each wave found in a staging turn, double-buffered over the turns
    int red[4];
};

// side `label` of image n: 0 = truth, 1 = pred.  Called with block-uniform arguments.
__device__ __forceinline__ HausSide haus_side(const Haus& t, int side, int n, int label) {
    const int cap = side ? t.cap_pred : t.cap_truth;
    const int32_t* box = (side ? t.box_pred : t.box_truth) + 4 * ((long long)n * cap + label - 1);
    return HausSide{(side ? t.pred : t.truth) + (long long)n * t.H * t.W, label, box[0], box[1], box[2], box[3]};
}

// The runs of b from item `it` of its box on (an item = 64 columns of one row of the box, one wave each, four per turn) into the
// stage, for as long as another turn is sure to fit (a wave finds at most 32 runs).  Returns the runs staged; `it` moves to the
// first item not taken.  Every thread of the workgroup calls it with the same arguments; it ends with a barrier.
__device__ __forceinline__ int haus_stage(const HausSide& b, int W, int& it, int items, int segs, HausLds& lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int count = 0, turn = 0;
    __syncthreads();                                                   // nobody still reads the stage
    for (; it < items && count + 4 * 32 <= kHausStage; it += 4, turn ^= 1) {
        const int item = it + wave;
        int row = 0, c = 0, len = 1;
        bool head = false;
        if (item < items) {
            row = b.r0 + item / segs;
            c = b.c0 + (item % segs) * 64 + lane;
            const bool live = c < b.c1 && b.img[(long long)row * W + c] == b.label;
            const unsigned long long bal = __ballot(live);
            head = bal && run_of(bal, 0ull, lane, len) && live;
        }
        const unsigned long long hb = __ballot(head);
        if (lane == 0) lds.heads[turn][wave] = __popcll(hb);
        __syncthreads();
        int at = count;
        for (int w = 0; w < 4; ++w) {
            const int k = lds.heads[turn][w];
            if (w < wave) at += k;
            count += k;
        }
        if (head) lds.run[at + __popcll(hb & ((1ull << lane) - 1))] = make_int2(row, (int)((unsigned)c | ((unsigned)(c + len - 1) << 16)));
    }
    __syncthreads();
    return count;
}

// d2(a -> b), the same value in every thread.  Every thread of the workgroup calls it with the same arguments.
__device__ int haus_directed(const HausSide& a, const HausSide& b, int W, HausLds& lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned aw = (unsigned)(a.c1 - a.c0), apix = aw * (unsigned)(a.r1 - a.r0);   // <= H W < 2^31: base below stays in 32 bits
    const int segs = (b.c1 - b.c0 + 63) >> 6, items = segs * (b.r1 - b.r0);
    int worst = 0, count = 0;
    bool whole = false;                                                // the stage holds all of b
    for (unsigned base = 0; base < apix; base += 256 * kHausPix) {
        int pr[kHausPix], pc[kHausPix], m[kHausPix];
        bool mine = false;
#pragma unroll
        for (int k = 0; k < kHausPix; ++k) {
            const unsigned idx = base + k * 256 + threadIdx.x;
            const bool in = idx < apix;
            pr[k] = a.r0 + (in ? (int)(idx / aw) : 0);
            pc[k] = a.c0 + (in ? (int)(idx % aw) : 0);
            const bool own = in && a.img[(long long)pr[k] * W + pc[k]] == a.label;
            m[k] = own ? INT_MAX : 0;                                  // a pixel that is not a's stays at 0: no part of the maximum
            mine |= own;
        }
        if (!__syncthreads_or(mine)) continue;
        const bool wave_mine = __ballot(mine) != 0;
        int it = 0;
        do {
            if (!whole) {
                const bool first = it == 0;
                count = haus_stage(b, W, it, items, segs, lds);
                whole = first && it >= items;
            }
            if (wave_mine) {
                for (int j = 0; j < count; ++j) {
                    const int2 u = lds.run[j];
                    const int c0 = u.y & 0xFFFF, c1 = (int)((unsigned)u.y >> 16);
#pragma unroll
                    for (int k = 0; k < kHausPix; ++k) {
                        const int dr = pr[k] - u.x, dc = max(max(c0 - pc[k], pc[k] - c1), 0);
                        m[k] = min(m[k], dr * dr + dc * dc);
                    }
                }
            }
        } while (!whole && it < items);
#pragma unroll
        for (int k = 0; k < kHausPix; ++k) worst = max(worst, m[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) worst = max(worst, __shfl_xor(worst, off));
    __syncthreads();                                                   // nobody still reads red from the call before
    if (lane == 0) lds.red[wave] = worst;
    __syncthreads();
    return max(max(lds.red[0], lds.red[1]), max(lds.red[2], lds.red[3]));
}

__device__ __forceinline__ int haus_h2(const HausSide& a, const HausSide& b, int W, HausLds& lds) {
    const int ab = haus_directed(a, b, W, lds);
    return max(ab, haus_directed(b, a, W, lds));
}

// row -> side (0 = truth, 1 = pred), image and label
__device__ __forceinline__ void haus_row(const Haus& t, long long row, int& side, int& n, int& label) {
    const long long nt = (long long)t.N * t.cap_truth;
    side = row >= nt;
    const long long i = side ? row - nt : row;
    const int cap = side ? t.cap_pred : t.cap_truth;
    n = (int)(i / cap);
    label = (int)(i - (long long)n * cap) + 1;
}

// One workgroup per row at a time.  No object: (0, -1).  An object whose given partner is an object of the other side: H2 with
// it.  Any other object goes on the list and gets (0, -1) for the time being.
__global__ __launch_bounds__(256) void hausdorff_partner_kernel(Haus t) {
    __shared__ HausLds lds;
    const long long rows = (long long)t.N * (t.cap_truth + t.cap_pred);
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        int side, n, label;
        haus_row(t, row, side, n, label);
        const long long nt = (long long)t.N * t.cap_truth;
        int32_t* partner = side ? t.partner_pred + (row - nt) : t.partner_truth + row;
        int32_t* d2 = side ? t.d2_pred + (row - nt) : t.d2_truth + row;
        const HausSide a = haus_side(t, side, n, label);
        int with = 0, dist = -1;
        if (a.r1 > 0) {
            const int given = side ? t.given_pred[row - nt] : t.given_truth[row];
            const int cap_other = side ? t.cap_truth : t.cap_pred;
            HausSide b{};
            if (given >= 1 && given <= cap_other) b = haus_side(t, side ^ 1, n, given);
            if (b.r1 > 0) {
                with = given;
                dist = haus_h2(a, b, t.W, lds);
            } else if (threadIdx.x == 0) {
                t.list[__hip_atomic_fetch_add(t.n_list, 1, __ATOMIC_RELAXED, kGlobal)] = (int)row;
            }
        }
        if (threadIdx.x == 0) {
            *partner = with;
            *d2 = dist;
        }
    }
}

// What the boxes alone say about H2(A, B).  Below: the topmost pixel of whichever object starts higher is at least the difference of
// the two top rows away from every pixel of the other, and likewise at the other three edges.  Above: no two pixels of the two
// objects are farther apart than the corners of the box that holds both.
__device__ __forceinline__ int haus_box_below(const int32_t* a, const int32_t* b) {
    const int dr = max(abs(a[0] - b[0]), abs(a[2] - b[2])), dc = max(abs(a[1] - b[1]), abs(a[3] - b[3]));
    return max(dr * dr, dc * dc);
}
__device__ __forceinline__ int haus_box_above(const int32_t* a, const int32_t* b) {
    const int dr = max(a[2], b[2]) - 1 - min(a[0], b[0]), dc = max(a[3], b[3]) - 1 - min(a[1], b[1]);
    return dr * dr + dc * dc;                                          // <= (H - 1)^2 + (W - 1)^2
}

// the box of label `cand` of the side opposite to row's, or NULL where that is no object
__device__ __forceinline__ const int32_t* haus_candidate_box(const Haus& t, int side, int n, int cand) {
    const int cap = side ? t.cap_truth : t.cap_pred;
    if (cand > cap) return nullptr;
    const int32_t* box = (side ? t.box_truth : t.box_pred) + 4 * ((long long)n * cap + cand - 1);
    return box[2] > 0 ? box : nullptr;
}

// One wave per (listed row, 64 labels of the other side) at a time: the smallest upper bound among the candidates into the row's
// bound.  The candidate that attains it has an H2 no larger, so the row's smallest H2 is no larger either.
__global__ __launch_bounds__(256) void hausdorff_bound_kernel(Haus t) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap_most = max(t.cap_pred, t.cap_truth), chunks = (cap_most + 63) >> 6;
    const long long jobs = (long long)*t.n_list * chunks;
    for (long long job = (long long)blockIdx.x * 4 + wave; job < jobs; job += (long long)gridDim.x * 4) {
        const long long row = t.list[job / chunks];
        int side, n, label;
        haus_row(t, row, side, n, label);
        const int32_t* a = (side ? t.box_pred : t.box_truth) + 4 * ((long long)n * (side ? t.cap_pred : t.cap_truth) + label - 1);
        const int32_t* b = haus_candidate_box(t, side, n, (int)(job % chunks) * 64 + lane + 1);
        int above = b ? haus_box_above(a, b) : INT_MAX;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) above = min(above, __shfl_xor(above, off));
        if (lane == 0 && above != INT_MAX) lower_to(t.bound + row, above);
    }
}

// One workgroup per (listed row, 256 labels of the other side) at a time.  Every thread holds one label against the row's object
// by their boxes: an object whose lower bound exceeds the row's bound, or the H2 of a candidate already done, cannot be the
// nearest nor tie with it, and is left out -- which candidates that spares depends on the order the jobs end in, the minimum does
// not.  The workgroup then takes the candidates that are left one by one: the H2 goes into the row's minimum of (H2 << 32) | label,
// the smallest distance and among equals the lowest label, in whatever order the jobs end.
__global__ __launch_bounds__(256) void hausdorff_candidate_kernel(Haus t) {
    __shared__ HausLds lds;
    __shared__ int left[256];
    __shared__ int wsum[4];
    const int cap_most = max(t.cap_pred, t.cap_truth), chunks = (cap_most + 255) >> 8;
    const long long jobs = (long long)*t.n_list * chunks;
    for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
        const long long row = t.list[job / chunks];
        const int cand = (int)(job % chunks) * 256 + (int)threadIdx.x + 1;
        int side, n, label;
        haus_row(t, row, side, n, label);
        const int32_t* mine = (side ? t.box_pred : t.box_truth) + 4 * ((long long)n * (side ? t.cap_pred : t.cap_truth) + label - 1);
        const int32_t* b = haus_candidate_box(t, side, n, cand);
        bool keep = false;
        if (b) {
            const unsigned done = (unsigned)(__hip_atomic_load(t.best + row, __ATOMIC_RELAXED, kGlobal) >> 32);   // none: all ones
            keep = (unsigned)haus_box_below(mine, b) <= min((unsigned)t.bound[row], done);
        }
        int n_left;
        const int at = block_rank<256>(keep, wsum, n_left);
        if (keep) left[at] = cand;
        __syncthreads();
        const HausSide a = haus_side(t, side, n, label);
        for (int i = 0; i < n_left; ++i) {
            const int c = left[i];
            const int dist = haus_h2(a, haus_side(t, side ^ 1, n, c), t.W, lds);
            if (threadIdx.x == 0)
                __hip_atomic_fetch_min(t.best + row, ((unsigned long long)(unsigned)dist << 32) | (unsigned)c, __ATOMIC_RELAXED, kGlobal);
        }
        __syncthreads();                                               // nobody still reads `left`
    }
}

// One thread per listed row: the winner into the tables (a row without a candidate keeps (0, -1)).
__global__ __launch_bounds__(256) void hausdorff_finish_kernel(Haus t) {
    const long long nt = (long long)t.N * t.cap_truth;
    const int listed = *t.n_list;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < listed; i += (long long)gridDim.x * 256) {
        const long long row = t.list[i];
        const unsigned long long b = t.best[row];
        if (b == ~0ull) continue;
        (row >= nt ? t.partner_pred + (row - nt) : t.partner_truth + row)[0] = (int)(unsigned)b;
        (row >= nt ? t.d2_pred + (row - nt) : t.d2_truth + row)[0] = (int)(b >> 32);
    }
}

// ---- seeded split ------------------------------------------------------------------------------------------------------------------
// One thread per point. A point is a live seed when it is one of the first S'_n of its image, lies inside the image and on a
// foreground pixel.  A live seed is pushed on the chain of its component: the root's slot of `head` (the spent cnt array) holds the
// area (> 0) while the component has no seed and -(p + 1), p = the point on top of the chain, afterwards; rec[p] = (row, col, index
// within the image, the next point of the chain or -1).  The order of a chain depends on the order the pushes land in; what the
// assign pass takes from it, the minimum of (d2, index) over the chain, does not.  keys (geodesic split, else NULL): a live seed also
// lowers the key of its pixel to (0, index).
__global__ __launch_bounds__(256) void seed_kernel(const uint8_t* __restrict__ m, int N, int H, int W, PointSet s,
                                                   const int32_t* __restrict__ lab, int32_t* __restrict__ head, int4* __restrict__ rec,
                                                   uint8_t* __restrict__ live, unsigned long long* __restrict__ keys) {
    const long long HW = (long long)H * W, total = HW * N;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < s.P; p += (long long)gridDim.x * 256) {
        const int n = point_image(s, N, p);
        bool ok = n >= 0;
        long long k = 0;                                               // the point's index within its image
        if (ok) {
            const PointWindow w = point_window(s, n);
            k = p - w.o0;
            ok = k < w.kept;
        }
        const long long r = s.pts[2 * p], c = s.pts[2 * p + 1];
        ok = ok && r >= 0 && r < H && c >= 0 && c < W;
        const long long q = ok ? n * HW + r * W + c : 0;
        ok = ok && m[q] != 0;
        live[p] = (uint8_t)ok;
        if (!ok) continue;
        const int root = lab[q];
        if ((unsigned)root >= (unsigned)total) continue;               // never with a workspace that label_into filled
        const int old = __hip_atomic_exchange(head + root, (int)(-(p + 1)), __ATOMIC_RELAXED, kGlobal);
        rec[p] = make_int4((int)r, (int)c, (int)k, old < 0 ? -old - 1 : -1);
        if (keys) atomicMin(keys + q, (unsigned long long)k);
    }
}

// 1 + the index of the seed of the chain from point q on that minimises (dr^2 + dc^2, index); d2 < 2^31 as H^2 + W^2 is.  A chain
// holds every point at most once, so P steps bound the walk.
__device__ __forceinline__ int nearest_seed(const int4* __restrict__ rec, int q, int P, int r, int c) {
    unsigned long long best = ~0ull;
    for (int step = 0; (unsigned)q < (unsigned)P && step < P; ++step) {
        const int4 s = rec[q];
        const int dr = r - s.x, dc = c - s.y;
        const unsigned long long key = ((unsigned long long)(unsigned)(dr * dr + dc * dc) << 32) | (unsigned)s.z;
        best = key < best ? key : best;
        q = s.w;
    }
    return (int)(unsigned)best + 1;
}

// head[root] > 0 is the label itself (a component without a seed, numbered by number_into<true>), < 0 the chain to walk.  Where
// every foreground lane of the wave has the same root (the inside of a cell clump, most waves) the chain is read through
// wave-uniform addresses and no lane diverges; otherwise every lane walks its own.  Background writes 0: the output needs no
// clearing.
__global__ __launch_bounds__(256) void split_assign_kernel(const uint8_t* __restrict__ m, int N, int H, int W,
                                                           const int32_t* __restrict__ lab, const int32_t* __restrict__ head,
                                                           const int4* __restrict__ rec, int P, int32_t* __restrict__ out) {
    const long long total = (long long)N * H * W;
    walk_row_segments(N, H, W, [&](int, int r, int c, long long p) {
        const bool fg = c < W && m[p] != 0;
        const unsigned long long bal = __ballot(fg);
        int label = 0;
        if (bal != 0) {
            int root = fg ? lab[p] : -1;
            if ((unsigned)root >= (unsigned)total) root = -1;          // never with a workspace that label_into filled
            const int x = root >= 0 ? head[root] : 0;
            const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(bal));
            const int root0 = __builtin_amdgcn_readlane(root, lead);
            if (__ballot(fg && root != root0) == 0) {
                const int x0 = __builtin_amdgcn_readlane(x, lead);
                const int l0 = x0 < 0 ? nearest_seed(rec, -x0 - 1, P, r, c) : x0;
                label = fg ? l0 : 0;
            } else if (fg) {
                label = x < 0 ? nearest_seed(rec, -x - 1, P, r, c) : x;
            }
        }
        if (c < W) out[p] = label;
    });
}

// ---- geodesic seeded split -----------------------------------------------------------------------------------------------------------
// Every foreground pixel holds one key, dist << 32 | k: the cheapest path found so far from a live seed to it (5 per axial and 7
// per diagonal step between foreground pixels of the 8-neighbourhood; CONN == 1: a diagonal step needs one of the two pixels it
// cuts between to be foreground, so that no step leaves a 4-component) and the index of that seed; all ones = not reached.  Keys
// only ever decrease and every value is the cost of a real path, so the fixpoint -- the minimum of (dist, k) over the live seeds of
// the pixel's component -- is the same whatever order the tiles run in.
constexpr int kGT = kT + 2;                                    // a tile and its one-pixel halo
constexpr unsigned long long kUnreached = ~0ull;
constexpr unsigned long long kStepAxial = 5ull << 32, kStepDiagonal = 7ull << 32;

__global__ __launch_bounds__(256) void geodesic_init_kernel(long long total, unsigned long long* __restrict__ keys) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) keys[p] = kUnreached;
}

// One round: grid (tiles across, tiles down, N), one workgroup per 64 x 64 tile.  The tile takes its keys and a one-pixel halo into
// LDS and sweeps until none of its keys changes: in a sweep every thread pulls, for each of its 16 pixels, the minimum over the
// allowed neighbours of key + step; a pixel's key is written by its owner only, after the barrier that ends the sweep's reads.  The
// halo stays as it was read.  Keys that fell go back with relaxed agent-scope atomic stores and the halo is read with the matching
// loads: a neighbouring tile may be writing in the same launch, and whatever it has written so far is the cost of a real path.
// A tile's byte of `next`: bit 0 = it lowered a key in this round, bit 1 = it holds foreground.  prev (NULL in the first round of
// a call, which runs every tile): the bytes of the round before; a tile runs only if it holds foreground and it or one of its
// eight neighbours lowered a key then -- otherwise its keys and its halo are what they were when it last found nothing to do.
template <int CONN>
__global__ __launch_bounds__(256) void geodesic_relax_kernel(const uint8_t* __restrict__ m, int H, int W, unsigned long long* keys,
                                                             const uint8_t* __restrict__ prev, uint8_t* __restrict__ next) {
    __shared__ unsigned long long key[kGT * kGT];
    __shared__ uint8_t val[kGT * kGT];
    const int tx = blockIdx.x, ty = blockIdx.y, nx = gridDim.x, ny = gridDim.y;
    const long long tile0 = (long long)blockIdx.z * ny * nx, tile = tile0 + (long long)ty * nx + tx;
    if (prev) {                                                // the same bytes for every thread: the whole workgroup leaves or stays
        const int own = prev[tile];
        int stirred = 0;
        if (own & 2)
            for (int y = max(ty - 1, 0); y <= min(ty + 1, ny - 1); ++y)
                for (int x = max(tx - 1, 0); x <= min(tx + 1, nx - 1); ++x) stirred |= prev[tile0 + (long long)y * nx + x] & 1;
        if (!stirred) {
            if (threadIdx.x == 0) next[tile] = (uint8_t)(own & 2);
            return;
        }
    }
    const int c0 = tx * kT, r0 = ty * kT;
    const long long img = (long long)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < kGT * kGT; i += 256) {
        const int r = r0 - 1 + i / kGT, c = c0 - 1 + i % kGT;
        const bool in = r >= 0 && r < H && c >= 0 && c < W;
        const long long p = img + (long long)r * W + c;
        const bool fg = in && m[p] != 0;
        val[i] = (uint8_t)fg;
        key[i] = fg ? __hip_atomic_load(keys + p, __ATOMIC_RELAXED, kGlobal) : kUnreached;
    }
    __syncthreads();
    unsigned long long cur[kPer], loaded[kPer];
    unsigned mine = 0;                                         // bit k: this thread's pixel k is foreground
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int j = ((i >> 6) + 1) * kGT + (i & 63) + 1;
        cur[k] = loaded[k] = key[j];
        mine |= (unsigned)val[j] << k;
    }
    if (!__syncthreads_or(mine != 0)) {                        // nothing to own here: never run again
        if (threadIdx.x == 0) next[tile] = 0;
        return;
    }
    // a path inside the tile and its halo has at most kTP steps, so kTP sweeps settle it; a tile that is cut short says it changed
    for (int sweep = 0; sweep < kTP; ++sweep) {
        unsigned fell = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (!((mine >> k) & 1)) continue;
            const int i = threadIdx.x + 256 * k;
            const int j = ((i >> 6) + 1) * kGT + (i & 63) + 1;
            unsigned long long best = cur[k];
            auto pull = [&](int q, unsigned long long step) {
                const unsigned long long v = key[q];
                if (v != kUnreached && v + step < best) best = v + step;
            };
            pull(j - 1, kStepAxial);
            pull(j + 1, kStepAxial);
            pull(j - kGT, kStepAxial);
            pull(j + kGT, kStepAxial);
            const bool up = CONN == 2 || val[j - kGT], down = CONN == 2 || val[j + kGT];
            const bool left = CONN == 2 || val[j - 1], right = CONN == 2 || val[j + 1];
            if (up || left) pull(j - kGT - 1, kStepDiagonal);
            if (up || right) pull(j - kGT + 1, kStepDiagonal);
            if (down || left) pull(j + kGT - 1, kStepDiagonal);
            if (down || right) pull(j + kGT + 1, kStepDiagonal);
            if (best < cur[k]) {
                cur[k] = best;
                fell |= 1u << k;
            }
        }
        __syncthreads();                                       // every read of this sweep is done
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int i = threadIdx.x + 256 * k;
            if ((fell >> k) & 1) key[((i >> 6) + 1) * kGT + (i & 63) + 1] = cur[k];
        }
        if (!__syncthreads_or(fell != 0)) break;
    }
    bool wrote = false;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (cur[k] >= loaded[k]) continue;                     // only a foreground pixel of the image ever falls
        const int i = threadIdx.x + 256 * k;
        __hip_atomic_store(keys + img + (long long)(r0 + (i >> 6)) * W + c0 + (i & 63), cur[k], __ATOMIC_RELAXED, kGlobal);
        wrote = true;
    }
    const int changed = __syncthreads_or(wrote);
    if (threadIdx.x == 0) next[tile] = (uint8_t)(changed ? 3 : 2);
}

// grid N.  last: the bytes of the last round run (NULL: no round was needed); converged[n] = no tile of image n lowered a key in it
__global__ __launch_bounds__(256) void geodesic_converged_kernel(const uint8_t* __restrict__ last, int tiles, uint8_t* __restrict__ converged) {
    int stirred = 0;
    if (last)
        for (int i = threadIdx.x; i < tiles; i += 256) stirred |= last[(long long)blockIdx.x * tiles + i] & 1;
    stirred = __syncthreads_or(stirred);
    if (threadIdx.x == 0) converged[blockIdx.x] = (uint8_t)(stirred == 0);
}

// head[root] > 0 is the label itself (a component without a live seed), < 0 the chain of a component that has one: its pixels take
// 1 + the seed of their key and its distance.  A pixel that no round has reached yet takes the seed on top of its component's chain
// and distance -1.  dist may be NULL.  Background writes 0 to both: the outputs need no clearing.
__global__ __launch_bounds__(256) void geodesic_assign_kernel(const uint8_t* __restrict__ m, int N, int H, int W,
                                                              const int32_t* __restrict__ lab, const int32_t* __restrict__ head,
                                                              const int4* __restrict__ rec, int P,
                                                              const unsigned long long* __restrict__ keys, int32_t* __restrict__ out,
                                                              int32_t* __restrict__ dist) {
    const long long total = (long long)N * H * W;
    walk_row_segments(N, H, W, [&](int, int, int c, long long p) {
        if (c >= W) return;
        int label = 0, d = 0;
        if (m[p] != 0) {
            const int root = lab[p];
            const int x = (unsigned)root < (unsigned)total ? head[root] : 0;       // in range with a workspace that label_into filled
            if (x > 0) {
                label = x;
                d = -1;
            } else if (x < 0) {
                const unsigned long long key = keys[p];
                const int q = -x - 1;
                if (key != kUnreached) {
                    label = (int)(unsigned)key + 1;
                    d = (int)(key >> 32);
                } else {
                    label = (unsigned)q < (unsigned)P ? rec[q].z + 1 : 0;
                    d = -1;
                }
            }
        }
        out[p] = label;
        if (dist) dist[p] = d;
    });
}

__global__ __launch_bounds__(256) void threshold_kernel(const float* __restrict__ p, long long n, float thr, uint8_t* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = (uint8_t)(p[i] > thr);
}

__global__ __launch_bounds__(256) void hsv_gate_kernel(const uint8_t* __restrict__ rgb, const uint8_t* mask, long long n, int v_max,
                                                       uint8_t* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const uint8_t* px = rgb + 3 * i;
        const int v = max(max((int)px[0], (int)px[1]), (int)px[2]);
        out[i] = (uint8_t)(mask[i] != 0 && v <= v_max);
    }
}

inline unsigned grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b < 1) b = 1;
    return (unsigned)(b > 16384 ? 16384 : b);
}
// the grid of a kernel that calls walk_row_segments(N, H, W, .)
inline dim3 walk_grid(int N, int H, int W) { return dim3(grid_for((long long)N * H * cs_ceil_div(W, 64) * 64)); }
inline long long blocks_per_image(int H, int W) { return ((long long)H * W + kNB - 1) / kNB; }

bool sizes_ok(int N, int H, int W) { return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31); }

int fail(const char* what, const char* why) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    cs_set_error_(msg);
    return CS_ERR_INVALID_ARG;
}

// A workspace is a row of arrays that each start on a 16-byte boundary.  A *_layout function takes the arrays of one workspace in
// order, writes their addresses where the kernels want them and returns the bytes in all: the one description of that workspace.
// The cs_regions_*_workspace entry calls it on a NULL base for the size, the entry point that runs on it on the caller's pointer.
struct Carve {
    uintptr_t base;
    size_t end = 0;
    template <typename T>
    T* take(size_t count) {
        T* at = reinterpret_cast<T*>(base + end);
        end += (count * sizeof(T) + 15) & ~(size_t)15;
        return at;
    }
};

struct Ws { int32_t *lab, *cnt, *blk; };
// lab, cnt (int32 N H W each), blk (int32 N ceil(H W / 1024)); with rec, for a split: then rec (int4 P)
size_t regions_layout(void* w, int N, int H, int W, Ws* ws, int P = 0, int4** rec = nullptr) {
    const size_t t = (size_t)N * H * W;
    Carve c{reinterpret_cast<uintptr_t>(w)};
    *ws = Ws{c.take<int32_t>(t), c.take<int32_t>(t), c.take<int32_t>((size_t)N * blocks_per_image(H, W))};
    if (rec) *rec = c.take<int4>(P);
    return c.end;
}

// a geodesic split: the split's arrays, then keys (uint64 N H W) and flags (uint8 2 N tiles: the two byte maps of the rounds)
struct Geo { unsigned long long* keys; uint8_t* flags; int tiles; };
bool geodesic_sizes_ok(int N, int H, int W, int P) { return sizes_ok(N, H, W) && P >= 0 && 7LL * H * W < (1LL << 31); }
size_t geodesic_layout(void* w, int N, int H, int W, int P, Ws* ws, int4** rec, Geo* g) {
    Carve c{reinterpret_cast<uintptr_t>(w), regions_layout(w, N, H, W, ws, P, rec)};
    g->tiles = cs_ceil_div(H, kT) * cs_ceil_div(W, kT);
    g->keys = c.take<unsigned long long>((size_t)N * H * W);
    g->flags = c.take<uint8_t>(2 * (size_t)N * g->tiles);
    return c.end;
}

// the vote counters per pred label: one per bit of the largest truth label
inline int vote_bits(int cap_truth) {
    int b = 1;
    while (b < 31 && (cap_truth >> b)) ++b;
    return b;
}
bool match_sizes_ok(int N, int cap_pred, int cap_truth) {
    return N > 0 && N <= 65535 && cap_pred >= 1 && cap_truth >= 1 && (long long)N * cap_pred * vote_bits(cap_truth) < (1LL << 31) &&
           (long long)N * cap_truth < (1LL << 31);
}
// vote (int32 N cap_pred B), cand (int32 N cap_pred), for the capacities of t, whose B it sets; 0 for capacities no call takes
size_t match_layout(void* w, int N, Match* t) {
    if (!match_sizes_ok(N, t->s.cap_pred, t->s.cap_truth)) return 0;
    t->B = vote_bits(t->s.cap_truth);
    const size_t rows = (size_t)N * t->s.cap_pred;
    Carve c{reinterpret_cast<uintptr_t>(w)};
    t->vote = c.take<int32_t>(rows * t->B);
    t->cand = c.take<int32_t>(rows);
    return c.end;
}

// the slots of one image's pair table: the smallest power of two >= 2 max_pairs; 0 for a max_pairs no call takes
inline long long pair_slots(int max_pairs) {
    if (max_pairs < 1 || max_pairs > (1 << 29)) return 0;
    long long s = 2;
    while (s < 2LL * max_pairs) s <<= 1;
    return s;
}
// The pair table at the head of a workspace: keys (uint64 N slots), then k int32 count arrays of N slots each, taken as one array
// at *counts (4 N slots need not be 16-byte aligned, 8 N slots is); sets p's slots.  false for sizes no call takes.  N slots is even,
// so the arrays are the first 8 N slots bytes and k times the next 4 N slots with no padding between them:
// kernels._pair_table_views (Python) views these (8 + 4 k) N slots bytes as the result's slot_keys / slot_<count>.
bool pair_table_layout(Carve* c, int N, int max_pairs, int k, PairTable* p, int32_t** counts) {
    const long long slots = pair_slots(max_pairs);
    if (!(N > 0 && N <= 65535 && slots > 0 && N * slots < (1LL << 31))) return false;
    p->slots = (int)slots;
    p->keys = c->take<unsigned long long>((size_t)N * slots);
    *counts = c->take<int32_t>((size_t)k * N * slots);
    return true;
}

// the pair table with cnt, then best_iou, best_it (uint64 N cap_truth each), best_ip (uint64 N cap_pred), for the capacities of t;
// 0 for sizes no call takes
size_t overlap_layout(void* w, int N, int max_pairs, Overlap* t) {
    Carve c{reinterpret_cast<uintptr_t>(w)};
    if (!pair_table_layout(&c, N, max_pairs, 1, &t->pairs, &t->cnt) || t->s.cap_pred < 1 || t->s.cap_truth < 1 ||
        (long long)N * t->s.cap_pred >= (1LL << 31) || (long long)N * t->s.cap_truth >= (1LL << 31))
        return 0;
    const size_t nt = (size_t)N * t->s.cap_truth;
    t->best_iou = c.take<unsigned long long>(nt);
    t->best_it = c.take<unsigned long long>(nt);
    t->best_ip = c.take<unsigned long long>((size_t)N * t->s.cap_pred);
    return c.end;
}

// the pair table with sides and corners, then best (uint64 N cap), for the capacity of t; 0 for sizes no call takes
size_t adjacency_layout(void* w, int N, int max_pairs, Adjacency* t) {
    Carve c{reinterpret_cast<uintptr_t>(w)};
    if (!pair_table_layout(&c, N, max_pairs, 2, &t->pairs, &t->sides) || t->cap < 1 || (long long)N * t->cap >= (1LL << 31)) return 0;
    t->corners = t->sides + (size_t)N * t->pairs.slots;
    t->best = c.take<unsigned long long>((size_t)N * t->cap);
    return c.end;
}

bool hausdorff_sizes_ok(int N, int H, int W, int cap_pred, int cap_truth) {
    return sizes_ok(N, H, W) && cap_pred >= 1 && cap_truth >= 1 && (long long)N * ((long long)cap_pred + cap_truth) < (1LL << 31) &&
           (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) < (1LL << 31);
}
// box_truth (int32 4 N cap_truth), box_pred (int32 4 N cap_pred), best (uint64 rows), list, bound (int32 rows each), n_list
// (int32 1), rows = N (cap_truth + cap_pred), for the capacities of t: 32 bytes per row and padding
size_t hausdorff_layout(void* w, Haus* t) {
    const size_t rows = (size_t)t->N * ((size_t)t->cap_truth + t->cap_pred);
    Carve c{reinterpret_cast<uintptr_t>(w)};
    t->box_truth = c.take<int32_t>(4 * (size_t)t->N * t->cap_truth);
    t->box_pred = c.take<int32_t>(4 * (size_t)t->N * t->cap_pred);
    t->best = c.take<unsigned long long>(rows);
    t->list = c.take<int32_t>(rows);
    t->bound = c.take<int32_t>(rows);
    t->n_list = c.take<int32_t>(1);
    return c.end;
}

// labels and areas of `m` into ws.lab / ws.cnt (cnt holds the area at every root's slot)
int label_into(const uint8_t* m, int N, int H, int W, int connectivity, const Ws& ws, hipStream_t st) {
    const dim3 tiles(cs_ceil_div(W, kT), cs_ceil_div(H, kT), N);
    const long long total = (long long)N * H * W;
    const long long edges = ((long long)((H - 1) / kT) * W + (long long)((W - 1) / kT) * H) * N;
    if (connectivity == 2) {
        hipLaunchKernelGGL(tile_label_kernel<2>, tiles, dim3(256), 0, st, m, H, W, ws.lab, ws.cnt);
        CS_LAUNCH_CHECK();
        if (edges > 0) hipLaunchKernelGGL(border_kernel<2>, dim3(grid_for(edges)), dim3(256), 0, st, m, N, H, W, ws.lab);
    } else {
        hipLaunchKernelGGL(tile_label_kernel<1>, tiles, dim3(256), 0, st, m, H, W, ws.lab, ws.cnt);
        CS_LAUNCH_CHECK();
        if (edges > 0) hipLaunchKernelGGL(border_kernel<1>, dim3(grid_for(edges)), dim3(256), 0, st, m, N, H, W, ws.lab);
    }
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(flatten_kernel, dim3(grid_for(total)), dim3(256), 0, st, total, ws.lab, ws.cnt);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

// scipy's number of every foreground root of ws.lab into its slot of ws.cnt (the areas there are spent); counts (or NULL): the
// number of foreground components of every image.  SEEDLESS (split, after the seed pass): only the roots without a seed, numbered
// from S'_n + 1, and counts = S'_n + their number.
template <bool SEEDLESS = false>
int number_into(const uint8_t* m, int N, int H, int W, const Ws& ws, int32_t* counts, hipStream_t st, const PointSet& seeds = PointSet{}) {
    const long long HW = (long long)H * W;
    const int B = (int)blocks_per_image(H, W);
    hipLaunchKernelGGL(number_count_kernel<SEEDLESS>, dim3(B, N), dim3(kNB), 0, st, m, ws.lab, ws.cnt, HW, ws.blk);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(number_scan_kernel, dim3(N), dim3(1024), 0, st, ws.blk, B, counts, seeds);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(number_assign_kernel<SEEDLESS>, dim3(B, N), dim3(kNB), 0, st, m, ws.lab, HW, ws.blk, ws.cnt, seeds);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

int carve(const char* what, int N, int H, int W, int connectivity, const void* in, const void* out, void* workspace, size_t bytes, Ws* ws) {
    if (!in || !out || !workspace) return fail(what, "NULL argument");
    if (!sizes_ok(N, H, W)) return fail(what, "need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    if (connectivity != 1 && connectivity != 2) return fail(what, "connectivity must be 1 or 2");
    if (bytes < regions_layout(workspace, N, H, W, ws)) return fail(what, "workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(what, "misaligned workspace");
    return CS_OK;
}

// What the two measure entry points check alike, after their own checks, and the tables as the kernels take them.
int tables_of(const char* what, const uint8_t* intensity, int32_t* area, int32_t* bbox, int64_t* sums, int64_t* isum, int32_t* imax,
              Tables* t) {
    if (intensity && !(isum && imax)) return fail(what, "an intensity image needs both intensity tables");
    if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(isum)) & 7) return fail(what, "misaligned int64 table");
    *t = Tables{area, bbox, reinterpret_cast<long long*>(sums), reinterpret_cast<long long*>(isum), imax};
    return CS_OK;
}

// What the entry points that take one or two label images and a workspace check alike.  given: every pointer of the entry is there;
// need: what its workspace layout returned, 0 for capacities it does not take, which is then the error caps_why.
int check_label_images(const char* what, bool given, int N, int H, int W, size_t need, const char* caps_why, const void* workspace,
                       size_t bytes) {
    if (!given) return fail(what, "NULL argument");
    if (!sizes_ok(N, H, W)) return fail(what, "need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    if (need == 0) return fail(what, caps_why);
    if (bytes < need) return fail(what, "workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(what, "misaligned workspace");
    return CS_OK;
}

}  // namespace

extern "C" size_t cs_regions_workspace(int N, int H, int W) {
    Ws ws;
    return sizes_ok(N, H, W) ? regions_layout(nullptr, N, H, W, &ws) : 0;
}

extern "C" int cs_regions_label(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* labels, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_label", N, H, W, connectivity, mask, labels, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
    if ((rc = number_into(mask, N, H, W, ws, nullptr, st)) != CS_OK) return rc;
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(spread_kernel, dim3(grid_for(N * HW)), dim3(256), 0, st, mask, N * HW, ws.lab, ws.cnt, 1, labels);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_number(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* counts, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_number", N, H, W, connectivity, mask, counts, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
    return number_into(mask, N, H, W, ws, counts, st);
}

extern "C" int cs_regions_measure(const uint8_t* mask, const uint8_t* intensity, int N, int H, int W, int connectivity, int capacity,
                                  int numbered, int32_t* counts, int32_t* area, int32_t* bbox, int64_t* sums, int64_t* isum,
                                  int32_t* imax, void* workspace, size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_measure", N, H, W, connectivity, mask, counts, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    CS_CHECK_ARG(area && bbox && sums, "regions_measure: NULL table");
    CS_CHECK_ARG(capacity >= 1 && capacity <= (long long)H * W, "regions_measure: need 1 <= capacity <= H W");
    CS_CHECK_ARG(numbered == 0 || numbered == 1, "regions_measure: numbered must be 0 or 1");
    Tables t;
    if ((rc = tables_of("regions_measure", intensity, area, bbox, sums, isum, imax, &t)) != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!numbered) {
        if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
        if ((rc = number_into(mask, N, H, W, ws, counts, st)) != CS_OK) return rc;
    }
    hipLaunchKernelGGL(measure_init_kernel, dim3(grid_for((long long)N * capacity)), dim3(256), 0, st, counts, N, capacity, t,
                       intensity ? 1 : 0, (int32_t*)nullptr);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(measure_kernel<false>, walk_grid(N, H, W), dim3(256), 0, st, mask, intensity, N, H, W, ws.lab, ws.cnt, capacity, t,
                       (int32_t*)nullptr);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_measure_labels(const int32_t* labels, const uint8_t* intensity, int N, int H, int W, int capacity,
                                         int32_t* counts, int32_t* area, int32_t* bbox, int64_t* sums, int64_t* isum, int32_t* imax,
                                         void* stream) {
    CS_CHECK_ARG(labels && area && bbox && sums, "regions_measure_labels: NULL argument");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_measure_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(capacity >= 1, "regions_measure_labels: need capacity >= 1");
    CS_CHECK_ARG((long long)N * capacity < (1LL << 31), "regions_measure_labels: need N capacity < 2^31");
    Tables t;
    const int rc = tables_of("regions_measure_labels", intensity, area, bbox, sums, isum, imax, &t);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long rows = (long long)N * capacity;
    hipLaunchKernelGGL(measure_init_kernel, dim3(grid_for(rows)), dim3(256), 0, st, (const int32_t*)nullptr, N, capacity, t,
                       intensity ? 1 : 0, counts);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(measure_kernel<true>, walk_grid(N, H, W), dim3(256), 0, st, (const uint8_t*)nullptr, intensity, N, H, W, labels,
                       (const int32_t*)nullptr, capacity, t, counts);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(measure_empty_rows_kernel, dim3(grid_for(rows)), dim3(256), 0, st, rows, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_edges_labels(const int32_t* labels, int N, int H, int W, uint8_t* edges, void* stream) {
    CS_CHECK_ARG(labels && edges, "regions_edges_labels: NULL argument");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_edges_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    hipLaunchKernelGGL(edge_kernel, walk_grid(N, H, W), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), labels, N, H, W, edges);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_shape_labels(const int32_t* labels, const uint8_t* edges, int N, int H, int W, int capacity, const int32_t* bbox,
                                       int64_t* moments, int32_t* tallies, void* stream) {
    CS_CHECK_ARG(labels && edges, "regions_shape_labels: NULL argument");
    CS_CHECK_ARG(bbox && moments && tallies, "regions_shape_labels: NULL table");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_shape_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(capacity >= 1, "regions_shape_labels: need capacity >= 1");
    CS_CHECK_ARG((long long)N * capacity < (1LL << 31), "regions_shape_labels: need N capacity < 2^31");
    CS_CHECK_ARG(H <= 32768 && W <= 32768, "regions_shape_labels: need H, W <= 32768 (the second moments are int64)");
    const ShapeTables t{bbox, reinterpret_cast<long long*>(moments), tallies};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long rows = (long long)N * capacity;
    hipLaunchKernelGGL(shape_init_kernel, dim3(grid_for(4 * rows)), dim3(256), 0, st, rows, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(shape_kernel, walk_grid(N, H, W), dim3(256), 0, st, labels, edges, N, H, W, capacity, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_stain_quantify_labels(const uint8_t* images_hwc, const int32_t* labels, const int32_t* expanded, int N, int H, int W,
                                        const int32_t* od_q, const int32_t* Mq, int K, const int32_t* pos_levels, int bins, int capacity,
                                        int32_t* counts, int32_t* n, int64_t* sum, int64_t* sumsq, int32_t* vmax, int32_t* pos,
                                        int32_t* hist, void* stream) {
    CS_CHECK_ARG(images_hwc && labels && od_q && Mq, "stain_quantify_labels: NULL argument");
    CS_CHECK_ARG(n && sum && sumsq && vmax && pos, "stain_quantify_labels: NULL table");
    CS_CHECK_ARG(sizes_ok(N, H, W), "stain_quantify_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(K == 2 || K == 3, "stain_quantify_labels: need K = 2 or 3 stains");
    CS_CHECK_ARG(bins == 0 || bins == 16 || bins == 32 || bins == 64 || bins == 128 || bins == 256,
                 "stain_quantify_labels: bins must be 0, 16, 32, 64, 128 or 256");
    CS_CHECK_ARG((bins == 0) == (hist == nullptr), "stain_quantify_labels: hist goes with bins > 0");
    CS_CHECK_ARG(capacity >= 1, "stain_quantify_labels: need capacity >= 1");
    const int C = expanded ? 2 : 1;
    CS_CHECK_ARG((long long)N * capacity * C * K * (bins ? bins : 1) < (1LL << 31), "stain_quantify_labels: need N capacity C K bins < 2^31");
    CS_CHECK_ARG(((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(expanded) | reinterpret_cast<uintptr_t>(od_q) |
                   reinterpret_cast<uintptr_t>(Mq)) & 3) == 0 && ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(sumsq)) & 7) == 0,
                 "stain_quantify_labels: misaligned argument");
    QuantTables t{n, reinterpret_cast<long long*>(sum), reinterpret_cast<long long*>(sumsq), vmax, pos, hist, counts, C, bins, {256, 256, 256}};
    for (int s = 0; s < K && pos_levels; ++s) {
        CS_CHECK_ARG(pos_levels[s] >= 0 && pos_levels[s] <= 256, "stain_quantify_labels: a positive level lies in [0, 256]");
        t.pos_level[s] = pos_levels[s];
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long slots = (long long)N * capacity * C;
    hipLaunchKernelGGL(quantify_init_kernel, dim3(grid_for(slots * K * (bins ? bins : 1))), dim3(256), 0, st, slots, K, N, t);
    CS_LAUNCH_CHECK();
    if (K == 2)
        hipLaunchKernelGGL(quantify_kernel<2>, walk_grid(N, H, W), dim3(256), 0, st, images_hwc, labels, expanded, N, H, W, od_q, Mq, capacity, t);
    else
        hipLaunchKernelGGL(quantify_kernel<3>, walk_grid(N, H, W), dim3(256), 0, st, images_hwc, labels, expanded, N, H, W, od_q, Mq, capacity, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_hull_max_side(void) { return kHullSide; }

extern "C" int cs_regions_hull_labels(const int32_t* labels, int N, int H, int W, int capacity, const int32_t* bbox, int32_t* hull,
                                      void* stream) {
    CS_CHECK_ARG(labels, "regions_hull_labels: NULL argument");
    CS_CHECK_ARG(bbox && hull, "regions_hull_labels: NULL table");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_hull_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(capacity >= 1, "regions_hull_labels: need capacity >= 1");
    CS_CHECK_ARG((long long)N * capacity < (1LL << 31), "regions_hull_labels: need N capacity < 2^31");
    const long long objects = (long long)N * capacity;
    hipLaunchKernelGGL(hull_kernel, dim3((unsigned)(objects < 8192 ? objects : 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       labels, N, H, W, capacity, bbox, hull);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_contour_max_side(void) { return kContourSide; }

extern "C" int cs_regions_contour_labels(const int32_t* labels, int N, int H, int W, int capacity, const int32_t* bbox, int connectivity,
                                         int max_vertices, int32_t* contour, int32_t* vertices, void* stream) {
    CS_CHECK_ARG(labels, "regions_contour_labels: NULL argument");
    CS_CHECK_ARG(bbox && contour, "regions_contour_labels: NULL table");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_contour_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(capacity >= 1, "regions_contour_labels: need capacity >= 1");
    CS_CHECK_ARG((long long)N * capacity < (1LL << 31), "regions_contour_labels: need N capacity < 2^31");
    CS_CHECK_ARG(connectivity == 1 || connectivity == 2, "regions_contour_labels: connectivity must be 1 or 2");
    CS_CHECK_ARG(max_vertices >= 0, "regions_contour_labels: need max_vertices >= 0");
    CS_CHECK_ARG(vertices || max_vertices == 0, "regions_contour_labels: NULL vertices with max_vertices > 0");
    const long long objects = (long long)N * capacity;
    CS_CHECK_ARG(2 * objects * max_vertices < (1LL << 31), "regions_contour_labels: need 2 N capacity max_vertices < 2^31");
    const dim3 grid((unsigned)(objects < 8192 ? objects : 8192));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (connectivity == 1)
        hipLaunchKernelGGL(contour_kernel<1>, grid, dim3(256), 0, st, labels, N, H, W, capacity, bbox, max_vertices, contour, vertices);
    else
        hipLaunchKernelGGL(contour_kernel<2>, grid, dim3(256), 0, st, labels, N, H, W, capacity, bbox, max_vertices, contour, vertices);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_texture_labels(const int32_t* labels, const uint8_t* plane, const uint8_t* images_hwc, const int32_t* od_q,
                                         const int32_t* Mq, int N, int H, int W, int capacity, const int32_t* bbox, int levels, int distance,
                                         int32_t* pairs, int32_t* diff, int32_t* sum, int32_t* marg, int64_t* sq, int64_t* cross,
                                         int32_t* matrix, void* stream) {
    CS_CHECK_ARG(labels, "regions_texture_labels: NULL argument");
    CS_CHECK_ARG((plane != nullptr) != (images_hwc != nullptr), "regions_texture_labels: exactly one of the plane and the RGB image is given");
    CS_CHECK_ARG((od_q != nullptr) == (images_hwc != nullptr) && (Mq != nullptr) == (images_hwc != nullptr),
                 "regions_texture_labels: od_q and Mq go with the RGB image");
    CS_CHECK_ARG(bbox && pairs && diff && sum && marg && sq && cross, "regions_texture_labels: NULL table");
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_texture_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG((long long)H * W <= (1LL << 30), "regions_texture_labels: need H W <= 2^30 (the counts are int32)");
    CS_CHECK_ARG(levels == 8 || levels == 16 || levels == 32, "regions_texture_labels: levels must be 8, 16 or 32");
    CS_CHECK_ARG(distance >= 1 && distance <= 8, "regions_texture_labels: distance must lie in [1, 8]");
    CS_CHECK_ARG(capacity >= 1, "regions_texture_labels: need capacity >= 1");
    const long long objects = (long long)N * capacity;
    CS_CHECK_ARG(objects * 4 * (2 * levels - 1) < (1LL << 31), "regions_texture_labels: need N capacity 4 (2 levels - 1) < 2^31");
    CS_CHECK_ARG(!matrix || objects * 4 * levels * levels < (1LL << 31), "regions_texture_labels: need N capacity 4 levels^2 < 2^31");
    CS_CHECK_ARG(((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(od_q) | reinterpret_cast<uintptr_t>(Mq) |
                   reinterpret_cast<uintptr_t>(bbox) | reinterpret_cast<uintptr_t>(pairs) | reinterpret_cast<uintptr_t>(diff) |
                   reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(marg) | reinterpret_cast<uintptr_t>(matrix)) & 3) == 0 &&
                 ((reinterpret_cast<uintptr_t>(sq) | reinterpret_cast<uintptr_t>(cross)) & 7) == 0,
                 "regions_texture_labels: misaligned argument");
    const TextureTables t{pairs, diff, sum, marg, reinterpret_cast<long long*>(sq), reinterpret_cast<long long*>(cross), matrix};
    const dim3 grid((unsigned)(objects < 8192 ? objects : 8192));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (plane)
        hipLaunchKernelGGL(texture_kernel<kTexPlane>, grid, dim3(256), 0, st, labels, plane, N, H, W, od_q, Mq, capacity, bbox, levels,
                           distance, t);
    else
        hipLaunchKernelGGL(texture_kernel<kTexRgb>, grid, dim3(256), 0, st, labels, images_hwc, N, H, W, od_q, Mq, capacity, bbox, levels,
                           distance, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_regions_match_workspace(int N, int cap_pred, int cap_truth) {
    Match t{{nullptr, nullptr, nullptr, nullptr, cap_pred, cap_truth}};
    return match_layout(nullptr, N, &t);
}

extern "C" int cs_regions_match_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                                       int32_t* counts_pred, int32_t* counts_truth, int32_t* area_pred, int32_t* area_truth,
                                       int32_t* match, int32_t* inter, int32_t* match_truth, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    Match t{{area_pred, area_truth, counts_pred, counts_truth, cap_pred, cap_truth}, match, inter, match_truth};
    const int rc = check_label_images("regions_match_labels",
                                      pred && truth && area_pred && area_truth && match && inter && match_truth && workspace, N, H, W,
                                      match_layout(workspace, N, &t),
                                      "need capacities >= 1, N cap_pred bit_length(cap_truth) < 2^31 and N cap_truth < 2^31", workspace,
                                      workspace_bytes);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long rows = (long long)N * cap_pred;
    const long long cells = rows * t.B > (long long)N * cap_truth ? rows * t.B : (long long)N * cap_truth;
    hipLaunchKernelGGL(match_init_kernel, dim3(grid_for(cells)), dim3(256), 0, st, N, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_walk_kernel<true>, walk_grid(N, H, W), dim3(256), 0, st, pred, truth, N, H, W, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_candidate_kernel, dim3(grid_for(rows)), dim3(256), 0, st, rows, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_walk_kernel<false>, walk_grid(N, H, W), dim3(256), 0, st, pred, truth, N, H, W, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_decide_kernel, dim3(grid_for(rows)), dim3(256), 0, st, rows, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_regions_overlap_workspace(int N, int cap_pred, int cap_truth, int max_pairs) {
    Overlap t{{nullptr, nullptr, nullptr, nullptr, cap_pred, cap_truth}};
    return overlap_layout(nullptr, N, max_pairs, &t);
}

extern "C" int cs_regions_overlap_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                                         int max_pairs, int32_t* counts_pred, int32_t* counts_truth, int32_t* area_pred,
                                         int32_t* area_truth, int32_t* n_pairs, int32_t* dropped, int32_t* iou_partner, int32_t* iou_inter,
                                         int32_t* inter_partner_truth, int32_t* inter_truth, int32_t* inter_partner_pred,
                                         int32_t* inter_pred, void* workspace, size_t workspace_bytes, void* stream) {
    Overlap t{{area_pred, area_truth, counts_pred, counts_truth, cap_pred, cap_truth}, {n_pairs, dropped}, iou_partner, iou_inter,
              inter_partner_truth, inter_truth, inter_partner_pred, inter_pred};
    const int rc = check_label_images("regions_overlap_labels",
                                      pred && truth && area_pred && area_truth && n_pairs && dropped && iou_partner && iou_inter &&
                                          inter_partner_truth && inter_truth && inter_partner_pred && inter_pred && workspace,
                                      N, H, W, overlap_layout(workspace, N, max_pairs, &t),
                                      "need capacities >= 1, 1 <= max_pairs <= 2^29, N cap_pred < 2^31, N cap_truth < 2^31 and N slots < 2^31",
                                      workspace, workspace_bytes);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long ns = (long long)N * t.pairs.slots, np = (long long)N * cap_pred, nt = (long long)N * cap_truth;
    const long long labels = np > nt ? np : nt;
    hipLaunchKernelGGL(overlap_init_kernel, dim3(grid_for(ns > labels ? ns : labels)), dim3(256), 0, st, N, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(overlap_walk_kernel, walk_grid(N, H, W), dim3(256), 0, st, pred, truth, N, H, W, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(overlap_reduce_kernel, dim3(grid_for(ns)), dim3(256), 0, st, ns, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(overlap_finish_kernel, dim3(grid_for(labels)), dim3(256), 0, st, N, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_regions_adjacency_workspace(int N, int capacity, int max_pairs) {
    Adjacency t{};
    t.cap = capacity;
    return adjacency_layout(nullptr, N, max_pairs, &t);
}

extern "C" int cs_regions_adjacency_labels(const int32_t* labels, int N, int H, int W, int capacity, int max_pairs, int connectivity,
                                           int32_t* counts, int32_t* n_pairs, int32_t* dropped, int32_t* n_neighbors, int32_t* contact,
                                           int32_t* background, int32_t* outside, int32_t* partner, int32_t* partner_sides,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    Adjacency t{counts, {n_pairs, dropped}, n_neighbors, contact, background, outside, partner, partner_sides};
    t.cap = capacity;
    const int rc = check_label_images("regions_adjacency_labels",
                                      labels && n_pairs && dropped && n_neighbors && contact && background && outside && partner &&
                                          partner_sides && workspace,
                                      N, H, W, adjacency_layout(workspace, N, max_pairs, &t),
                                      "need capacity >= 1, 1 <= max_pairs <= 2^29, N capacity < 2^31 and N slots < 2^31", workspace,
                                      workspace_bytes);
    if (rc != CS_OK) return rc;
    if (connectivity != 1 && connectivity != 2) return fail("regions_adjacency_labels", "connectivity must be 1 or 2");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long ns = (long long)N * t.pairs.slots, rows = (long long)N * capacity;
    hipLaunchKernelGGL(adjacency_init_kernel, dim3(grid_for(ns > rows ? ns : rows)), dim3(256), 0, st, N, t);
    CS_LAUNCH_CHECK();
    if (connectivity == 2)
        hipLaunchKernelGGL(adjacency_walk_kernel<2>, walk_grid(N, H, W), dim3(256), 0, st, labels, N, H, W, t);
    else
        hipLaunchKernelGGL(adjacency_walk_kernel<1>, walk_grid(N, H, W), dim3(256), 0, st, labels, N, H, W, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(adjacency_reduce_kernel, dim3(grid_for(ns)), dim3(256), 0, st, ns, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(adjacency_finish_kernel, dim3(grid_for(rows)), dim3(256), 0, st, rows, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_seed_labels(const int64_t* points, const int64_t* offsets, const int32_t* limits, long long P, int N, int H,
                                      int W, int32_t* labels, void* stream) {
    CS_CHECK_ARG(sizes_ok(N, H, W), "regions_seed_labels: need 0 < N <= 65535, H, W > 0 and N H W < 2^31");
    CS_CHECK_ARG(P >= 0 && P < (1LL << 31), "regions_seed_labels: need 0 <= P < 2^31 rows");
    CS_CHECK_ARG(offsets && labels && (points || P == 0), "regions_seed_labels: NULL argument");
    CS_CHECK_ARG(((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(offsets)) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(labels) & 3) == 0, "regions_seed_labels: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PointSet s = {points, offsets, limits, P, 0};
    const long long total = (long long)N * H * W;
    hipLaunchKernelGGL(zero_labels_kernel, dim3(grid_for(total)), dim3(256), 0, st, total, labels);
    CS_LAUNCH_CHECK();
    if (P > 0) {
        hipLaunchKernelGGL(seed_labels_kernel<true>, dim3(grid_for(P)), dim3(256), 0, st, s, N, H, W, labels);
        CS_LAUNCH_CHECK();
        hipLaunchKernelGGL(seed_labels_kernel<false>, dim3(grid_for(P)), dim3(256), 0, st, s, N, H, W, labels);
        CS_LAUNCH_CHECK();
    }
    return CS_OK;
}

extern "C" int cs_regions_hausdorff_stage_runs(void) { return kHausStage; }

extern "C" size_t cs_regions_hausdorff_workspace(int N, int cap_pred, int cap_truth) {
    Haus t{};
    t.N = N, t.cap_pred = cap_pred, t.cap_truth = cap_truth;
    return hausdorff_sizes_ok(N, 1, 1, cap_pred, cap_truth) ? hausdorff_layout(nullptr, &t) : 0;
}

extern "C" int cs_regions_hausdorff_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                                           const int32_t* inter_partner_truth, const int32_t* inter_partner_pred, int32_t* partner_truth,
                                           int32_t* d2_truth, int32_t* partner_pred, int32_t* d2_pred, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    Haus t{pred, truth, inter_partner_truth, inter_partner_pred, partner_truth, d2_truth, partner_pred, d2_pred};
    t.N = N, t.H = H, t.W = W, t.cap_pred = cap_pred, t.cap_truth = cap_truth;
    const bool ok = sizes_ok(N, H, W) && hausdorff_sizes_ok(N, H, W, cap_pred, cap_truth);
    const int rc = check_label_images("regions_hausdorff_labels",
                                      pred && truth && inter_partner_truth && inter_partner_pred && partner_truth && d2_truth &&
                                          partner_pred && d2_pred && workspace,
                                      N, H, W, ok ? hausdorff_layout(workspace, &t) : 0,
                                      "need capacities >= 1, N (cap_pred + cap_truth) < 2^31 and (H - 1)^2 + (W - 1)^2 < 2^31", workspace,
                                      workspace_bytes);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long rows = (long long)N * ((long long)cap_pred + cap_truth);
    const int cap_most = cap_pred > cap_truth ? cap_pred : cap_truth;
    const long long by64 = rows * ((cap_most + 63) / 64), by256 = rows * ((cap_most + 255) / 256);
    hipLaunchKernelGGL(hausdorff_init_kernel, dim3(grid_for(rows)), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hausdorff_box_kernel, walk_grid(N, H, W), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hausdorff_partner_kernel, dim3((unsigned)(rows < 8192 ? rows : 8192)), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hausdorff_bound_kernel, dim3(grid_for(by64 * 64)), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hausdorff_candidate_kernel, dim3((unsigned)(by256 < 4096 ? by256 : 4096)), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hausdorff_finish_kernel, dim3(grid_for(rows)), dim3(256), 0, st, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_regions_split_workspace(int N, int H, int W, int P) {
    Ws ws;
    int4* rec;
    return sizes_ok(N, H, W) && P >= 0 ? regions_layout(nullptr, N, H, W, &ws, P, &rec) : 0;
}

extern "C" int cs_regions_split(const uint8_t* mask, int N, int H, int W, int connectivity, const int64_t* points, const int64_t* offsets,
                                const int32_t* limits, int P, int32_t* labels, int32_t* counts, uint8_t* live, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_split", N, H, W, connectivity, mask, labels, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    CS_CHECK_ARG(counts, "regions_split: NULL counts");
    CS_CHECK_ARG(P >= 0 && (P == 0 || (points && offsets && live)), "regions_split: P points need points, offsets and live");
    CS_CHECK_ARG((long long)H * H + (long long)W * W < (1LL << 31), "regions_split: need H^2 + W^2 < 2^31");
    CS_CHECK_ARG((long long)P + (long long)H * W < (1LL << 31), "regions_split: need P + H W < 2^31");
    int4* rec;
    CS_CHECK_ARG(workspace_bytes >= regions_layout(workspace, N, H, W, &ws, P, &rec), "regions_split: workspace too small");
    CS_CHECK_ARG(!((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(offsets)) & 7), "regions_split: misaligned int64 array");
    const PointSet seeds{points, P > 0 ? offsets : nullptr, limits, P, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
    if (P > 0) {
        hipLaunchKernelGGL(seed_kernel, dim3(grid_for(P)), dim3(256), 0, st, mask, N, H, W, seeds, ws.lab, ws.cnt, rec, live, nullptr);
        CS_LAUNCH_CHECK();
    }
    if ((rc = number_into<true>(mask, N, H, W, ws, counts, st, seeds)) != CS_OK) return rc;
    hipLaunchKernelGGL(split_assign_kernel, walk_grid(N, H, W), dim3(256), 0, st, mask, N, H, W, ws.lab, ws.cnt, rec, P, labels);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_regions_geodesic_workspace(int N, int H, int W, int P) {
    Ws ws;
    int4* rec;
    Geo g;
    return geodesic_sizes_ok(N, H, W, P) ? geodesic_layout(nullptr, N, H, W, P, &ws, &rec, &g) : 0;
}

extern "C" int cs_regions_split_geodesic(const uint8_t* mask, int N, int H, int W, int connectivity, const int64_t* points,
                                         const int64_t* offsets, const int32_t* limits, int P, int rounds, int resume, int32_t* labels,
                                         int32_t* counts, uint8_t* live, int32_t* distance, uint8_t* converged, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_split_geodesic", N, H, W, connectivity, mask, labels, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    CS_CHECK_ARG(counts, "regions_split_geodesic: NULL counts");
    CS_CHECK_ARG(converged, "regions_split_geodesic: NULL converged");
    CS_CHECK_ARG(P >= 0 && (P == 0 || (points && offsets && live)), "regions_split_geodesic: P points need points, offsets and live");
    CS_CHECK_ARG(rounds >= 1, "regions_split_geodesic: need rounds >= 1");
    CS_CHECK_ARG(7LL * H * W < (1LL << 31), "regions_split_geodesic: need 7 H W < 2^31");
    CS_CHECK_ARG((long long)P + (long long)H * W < (1LL << 31), "regions_split_geodesic: need P + H W < 2^31");
    int4* rec;
    Geo g;
    CS_CHECK_ARG(workspace_bytes >= geodesic_layout(workspace, N, H, W, P, &ws, &rec, &g), "regions_split_geodesic: workspace too small");
    CS_CHECK_ARG(!((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(offsets)) & 7),
                 "regions_split_geodesic: misaligned int64 array");
    const PointSet seeds{points, P > 0 ? offsets : nullptr, limits, P, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long total = (long long)N * H * W;
    if (!resume) {
        if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
        hipLaunchKernelGGL(geodesic_init_kernel, dim3(grid_for(total)), dim3(256), 0, st, total, g.keys);
        CS_LAUNCH_CHECK();
        if (P > 0) {
            hipLaunchKernelGGL(seed_kernel, dim3(grid_for(P)), dim3(256), 0, st, mask, N, H, W, seeds, ws.lab, ws.cnt, rec, live, g.keys);
            CS_LAUNCH_CHECK();
        }
        if ((rc = number_into<true>(mask, N, H, W, ws, counts, st, seeds)) != CS_OK) return rc;
    }
    const dim3 tiles(cs_ceil_div(W, kT), cs_ceil_div(H, kT), N);
    uint8_t* const map[2] = {g.flags, g.flags + (size_t)N * g.tiles};
    for (int t = 0; P > 0 && t < rounds; ++t) {                // without a point no key is ever set: nothing to relax
        const uint8_t* prev = t == 0 ? nullptr : map[(t - 1) & 1];
        if (connectivity == 2)
            hipLaunchKernelGGL(geodesic_relax_kernel<2>, tiles, dim3(256), 0, st, mask, H, W, g.keys, prev, map[t & 1]);
        else
            hipLaunchKernelGGL(geodesic_relax_kernel<1>, tiles, dim3(256), 0, st, mask, H, W, g.keys, prev, map[t & 1]);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(geodesic_converged_kernel, dim3(N), dim3(256), 0, st, P > 0 ? map[(rounds - 1) & 1] : nullptr, g.tiles, converged);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(geodesic_assign_kernel, walk_grid(N, H, W), dim3(256), 0, st, mask, N, H, W, ws.lab, ws.cnt, rec, P, g.keys, labels,
                       distance);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_areas(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* areas, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_areas", N, H, W, connectivity, mask, areas, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
    const long long total = (long long)N * H * W;
    hipLaunchKernelGGL(spread_kernel, dim3(grid_for(total)), dim3(256), 0, st, mask, total, ws.lab, ws.cnt, 0, areas);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_filter(const uint8_t* mask, int N, int H, int W, int connectivity, int value, int min_area, uint8_t* out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    Ws ws;
    int rc = carve("regions_filter", N, H, W, connectivity, mask, out, workspace, workspace_bytes, &ws);
    if (rc != CS_OK) return rc;
    CS_CHECK_ARG((value == 0 || value == 1) && min_area >= 0, "regions_filter: value must be 0 or 1 and min_area non-negative");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = label_into(mask, N, H, W, connectivity, ws, st)) != CS_OK) return rc;
    const long long total = (long long)N * H * W;
    hipLaunchKernelGGL(filter_kernel, dim3(grid_for(total)), dim3(256), 0, st, mask, total, ws.lab, ws.cnt, value, min_area, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_remove_small(const uint8_t* mask, int N, int H, int W, int min_object_size, int hole_area_threshold,
                                       int connectivity, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = cs_regions_filter(mask, N, H, W, connectivity, 1, min_object_size, out, workspace, workspace_bytes, stream);
    if (rc != CS_OK) return rc;
    return cs_regions_filter(out, N, H, W, connectivity, 0, hole_area_threshold, out, workspace, workspace_bytes, stream);
}

extern "C" int cs_regions_threshold(const float* probs, long long n, float threshold, uint8_t* out, void* stream) {
    CS_CHECK_ARG(probs && out && n > 0, "regions_threshold: bad arguments");
    hipLaunchKernelGGL(threshold_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), probs, n, threshold, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_regions_hsv_gate(const uint8_t* images_hwc, const uint8_t* mask, long long n_pixels, int v_max, uint8_t* out,
                                   void* stream) {
    CS_CHECK_ARG(images_hwc && mask && out && n_pixels > 0, "regions_hsv_gate: bad arguments");
    hipLaunchKernelGGL(hsv_gate_kernel, dim3(grid_for(n_pixels)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), images_hwc, mask,
                       n_pixels, v_max, out);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
