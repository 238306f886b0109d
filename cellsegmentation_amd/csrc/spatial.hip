// Neighbourhood queries over integer points: a bucket grid per image and three exact queries on top of it (spatial.py is the public
// API).  Points are the ragged point set of cs_points.h; a point is LIVE when its image's window keeps it (point_window) and it
// lies inside [0, H) x [0, W).  Only live points ask or answer.  With H^2 + W^2 < 2^31 every squared distance fits an int32 and the
// key (d2 << 32) | index fits 64 bits; every result is a minimum of distinct keys or a sum of integers, so nothing depends on the
// order in which points arrive in a bucket.
//
// Build, per point set (the queries; in cross mode the targets too), on square buckets of side b, nbr x nbc per image:
//   count    one thread per row of the buffer: the row's image by bisection of the offsets, one integer atomic per live point
//   scan     one workgroup per image: exclusive scan of the bucket counts (block_scan_incl, looping over the buckets 256 at a time)
//            into start[n][0 .. nb], start[n][nb] = the image's live points; the counts are zeroed again to serve as cursors
//   scatter  the count pass again: slot = start + cursor++, one 16-byte record (row, col, index within the image, 0) per live point,
//            image n's records from its first row on -- a bucket row-major, so a ROW of buckets is one contiguous span of records
// Queries: one workgroup of 256 threads per bucket of query points (an empty bucket returns at once), thread t holding query t, t +
// 256, ... of the bucket in turn; candidate spans are staged through LDS kChunk records at a time and read by every lane at once.
//   nearest       square rings of buckets around the query's bucket.  After ring q the scanned region is the bucket rows and columns
//                 within q of the query's; an unseen point is at least m away, m = the smallest gap from the query to the first row
//                 or column outside the region (sides on the image's border have none).  The query is settled when its k-th key
//                 has d2 < m^2 -- strictly: an unseen point AT m with a lower index would win the tie -- or when no side is left.
//                 The ring loop is uniform: it goes on while any thread is unsettled (__syncthreads_or).
//   count_within  the bucket rows and columns that cover [r - R, r + R] x [c - R, c + R] of every query of the bucket, R = isqrt of
//                 the largest radius2; |dr| > R or |dc| > R is rejected before anything is squared.  Per-image sums by one 64-bit
//                 integer atomic per workgroup and radius.
//   cluster       DBSCAN on the same box walk (walk_box), three times at the one radius: the passes are listed at the kernels.
// Launch geometry depends on (P, N, H, W, b, k) only; nothing synchronises with the host.
#include <limits.h>
#include "cs_common.h"
#include "cs_block.h"
#include "cs_points.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 512;                        // candidate records staged in LDS at a time
constexpr long long kMaxBuckets = 1LL << 22;       // N * nbr * nbc of one call
constexpr int kMaxRadii = 8, kMaxK = 8;
constexpr unsigned long long kNoKey = ~0ull;

struct Grid {
    int N, H, W, b, nbr, nbc, nb;                  // nb = nbr * nbc
};
struct Cells {
    int32_t* cnt;                                  // [N][nb]   counts, then cursors
    int32_t* start;                                // [N][nb + 1]
    int4* rec;                                     // [P]
};
struct Radii {
    int r2[kMaxRadii];
};

// the live point in row i of the buffer: image, index within it, bucket; false = the row holds none
struct Live {
    int n, idx, r, c, bk;
    long long o0;
};
__device__ __forceinline__ bool live_point(const PointSet& p, const Grid& g, long long i, Live& v) {
    const int n = point_image(p, g.N, i);
    if (n < 0) return false;
    const PointWindow w = point_window(p, n);
    if (i - w.o0 >= w.kept) return false;
    const long long r = p.pts[2 * i + p.xy], c = p.pts[2 * i + 1 - p.xy];
    if (r < 0 || r >= g.H || c < 0 || c >= g.W) return false;
    v.n = n;
    v.idx = (int)(i - w.o0);
    v.r = (int)r;
    v.c = (int)c;
    v.bk = ((int)r / g.b) * g.nbc + (int)c / g.b;
    v.o0 = w.o0;
    return true;
}

// grid-stride fill of n int32 words
__global__ __launch_bounds__(kThreads) void spatial_fill_kernel(int32_t* __restrict__ p, long long n, int v) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) p[i] = v;
}

// grid (ceil(P / 256)).  SCATTER = false: cnt[n][bucket] += 1 per live point.  true: the record into its bucket's next free slot.
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void spatial_count_kernel(PointSet p, Grid g, Cells cells) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.P) return;
    Live v;
    if (!live_point(p, g, i, v)) return;
    const int at = atomicAdd(cells.cnt + (long long)v.n * g.nb + v.bk, 1);
    if (SCATTER) cells.rec[v.o0 + cells.start[(long long)v.n * (g.nb + 1) + v.bk] + at] = make_int4(v.r, v.c, v.idx, 0);
}

// grid (N): start[n][j] = the live points of image n in the buckets before j, start[n][nb] = all of them; cnt[n][*] = 0 again
__global__ __launch_bounds__(kThreads) void spatial_scan_kernel(Grid g, Cells cells) {
    __shared__ int s_scan[kThreads];
    const int n = blockIdx.x, tid = threadIdx.x;
    int32_t* cnt = cells.cnt + (long long)n * g.nb;
    int32_t* start = cells.start + (long long)n * (g.nb + 1);
    int carry = 0;
    for (int j0 = 0; j0 < g.nb; j0 += kThreads) {
        const int j = j0 + tid;
        const int v = j < g.nb ? cnt[j] : 0;
        int total;
        const int incl = block_scan_incl<kThreads, int>(v, s_scan, total);
        if (j < g.nb) {
            start[j] = carry + incl - v;
            cnt[j] = 0;
        }
        carry += total;
    }
    if (tid == 0) start[g.nb] = carry;
}

// the records [s0, s1) of one image, kChunk at a time: every thread of the workgroup calls it (barriers); f(record) runs on the
// threads with `have` for every record
template <typename F>
__device__ __forceinline__ void scan_records(const int4* __restrict__ rec, int s0, int s1, int4* s_rec, bool have, F f) {
    for (int c0 = s0; c0 < s1; c0 += kChunk) {
        const int m = min(kChunk, s1 - c0);
        __syncthreads();                           // the chunk before this one has been read
        for (int e = threadIdx.x; e < m; e += kThreads) s_rec[e] = rec[c0 + e];
        __syncthreads();
        if (have)
            for (int e = 0; e < m; ++e) f(s_rec[e]);
    }
}

// the records of buckets [j0, j1] (one row of buckets, or part of one) of a target image
__device__ __forceinline__ void bucket_span(const int32_t* __restrict__ start, int j0, int j1, int& s0, int& s1) {
    s0 = start[j0];
    s1 = start[j1 + 1];
}

struct Query {
    const int32_t* q_start;                        // the query image's start row
    const int4* q_rec;                             // its records
    const int32_t* t_start;                        // the target image's
    const int4* t_rec;
    long long q_row0;                              // first row of the query image in the buffer
    int br, bc, q0, qn;                            // this workgroup's bucket and its records [q0, q0 + qn) of q_rec
};
__device__ __forceinline__ bool open_query(const PointSet& q, const PointSet& t, const Grid& g, const Cells& qc, const Cells& tc, Query& u) {
    const int n = blockIdx.x / g.nb, bk = blockIdx.x - n * g.nb;
    u.q_start = qc.start + (long long)n * (g.nb + 1);
    u.q0 = u.q_start[bk];
    u.qn = u.q_start[bk + 1] - u.q0;
    if (u.qn <= 0) return false;
    u.q_row0 = point_window(q, n).o0;
    u.q_rec = qc.rec + u.q_row0;
    u.t_start = tc.start + (long long)n * (g.nb + 1);
    u.t_rec = tc.rec + point_window(t, n).o0;
    u.br = bk / g.nbc;
    u.bc = bk - u.br * g.nbc;
    return true;
}

// grid (N * nb).  K in {1, 2, 4, 8} keys per thread, the first k written; SELF: queries and targets are one set, a row is never
// its own neighbour.
template <int K, bool SELF>
__global__ __launch_bounds__(kThreads) void spatial_nearest_kernel(PointSet q, PointSet t, Grid g, Cells qc, Cells tc, int k,
                                                                   int32_t* __restrict__ index, int32_t* __restrict__ d2_out) {
    __shared__ int4 s_rec[kChunk];
    Query u;
    if (!open_query(q, t, g, qc, tc, u)) return;
    const int b = g.b;
    for (int p0 = 0; p0 < u.qn; p0 += kThreads) {
        const bool have = p0 + (int)threadIdx.x < u.qn;
        const int4 me = have ? u.q_rec[u.q0 + p0 + threadIdx.x] : make_int4(0, 0, -1, 0);
        unsigned long long key[K];
#pragma unroll
        for (int j = 0; j < K; ++j) key[j] = kNoKey;
        auto take = [&](const int4& c) {
            if (SELF && c.z == me.z) return;
            const int dr = c.x - me.x, dc = c.y - me.y;
            const unsigned long long cand = ((unsigned long long)(uint32_t)(dr * dr + dc * dc) << 32) | (uint32_t)c.z;
            if (cand >= key[K - 1]) return;
            key[K - 1] = cand;
#pragma unroll
            for (int j = K - 1; j > 0; --j) {
                const unsigned long long lo = key[j] < key[j - 1] ? key[j] : key[j - 1];
                const unsigned long long hi = key[j] < key[j - 1] ? key[j - 1] : key[j];
                key[j - 1] = lo;
                key[j] = hi;
            }
        };
        for (int ring = 0;; ++ring) {
            const int r_lo = u.br - ring, r_hi = u.br + ring, c_lo = u.bc - ring, c_hi = u.bc + ring;
            const int cc_lo = max(c_lo, 0), cc_hi = min(c_hi, g.nbc - 1);
            int s0, s1;
            if (r_lo >= 0) {                                               // the ring's top row (ring 0: the bucket itself)
                bucket_span(u.t_start, r_lo * g.nbc + cc_lo, r_lo * g.nbc + cc_hi, s0, s1);
                scan_records(u.t_rec, s0, s1, s_rec, have, take);
            }
            if (ring > 0 && r_hi < g.nbr) {                                // its bottom row
                bucket_span(u.t_start, r_hi * g.nbc + cc_lo, r_hi * g.nbc + cc_hi, s0, s1);
                scan_records(u.t_rec, s0, s1, s_rec, have, take);
            }
            for (int rr = max(r_lo + 1, 0); rr <= min(r_hi - 1, g.nbr - 1); ++rr) {     // its two columns in between
                if (c_lo >= 0) {
                    bucket_span(u.t_start, rr * g.nbc + c_lo, rr * g.nbc + c_lo, s0, s1);
                    scan_records(u.t_rec, s0, s1, s_rec, have, take);
                }
                if (c_hi < g.nbc) {
                    bucket_span(u.t_start, rr * g.nbc + c_hi, rr * g.nbc + c_hi, s0, s1);
                    scan_records(u.t_rec, s0, s1, s_rec, have, take);
                }
            }
            // m = the smallest gap to a row or column not scanned yet; sides on the border of the image have none
            long long m = LLONG_MAX;
            if (r_lo > 0) m = min(m, (long long)me.x - (long long)r_lo * b + 1);
            if (r_hi < g.nbr - 1) m = min(m, (long long)(r_hi + 1) * b - me.x);
            if (c_lo > 0) m = min(m, (long long)me.y - (long long)c_lo * b + 1);
            if (c_hi < g.nbc - 1) m = min(m, (long long)(c_hi + 1) * b - me.y);
            unsigned long long kth = key[K - 1];                           // selects, not an indexed read: the keys stay in registers
#pragma unroll
            for (int j = 0; j < K - 1; ++j) kth = j == k - 1 ? key[j] : kth;
            const bool settled = m == LLONG_MAX || (kth != kNoKey && (long long)(kth >> 32) < m * m);
            if (!__syncthreads_or(have && !settled)) break;
        }
        if (have) {
            const long long row = u.q_row0 + me.z;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) {
                    const bool found = key[j] != kNoKey;
                    index[row * k + j] = found ? (int)(uint32_t)key[j] : -1;
                    d2_out[row * k + j] = found ? (int)(key[j] >> 32) : -1;
                }
        }
    }
}

// The box walk of the radius queries: every query `me` of the workgroup's bucket, 256 at a time, meets every target record of the
// bucket rows and columns that cover the reach `box` (pixels) around the bucket.  Every thread of the workgroup calls it (barriers);
// on the threads that hold a query, begin(me), then take(me, record) for every record of the box, then done(me, buffer row of me).
template <typename Begin, typename Take, typename Done>
__device__ __forceinline__ void walk_box(const Query& u, const Grid& g, int box, int4* s_rec, Begin begin, Take take, Done done) {
    const int b = g.b;
    const int br0 = max(u.br * b - box, 0) / b, br1 = (int)min(((long long)(u.br + 1) * b - 1 + box) / b, (long long)g.nbr - 1);
    const int bc0 = max(u.bc * b - box, 0) / b, bc1 = (int)min(((long long)(u.bc + 1) * b - 1 + box) / b, (long long)g.nbc - 1);
    for (int p0 = 0; p0 < u.qn; p0 += kThreads) {
        const bool have = p0 + (int)threadIdx.x < u.qn;
        const int4 me = have ? u.q_rec[u.q0 + p0 + threadIdx.x] : make_int4(0, 0, -1, 0);
        if (have) begin(me);
        for (int rr = br0; rr <= br1; ++rr) {
            int s0, s1;
            bucket_span(u.t_start, rr * g.nbc + bc0, rr * g.nbc + bc1, s0, s1);
            scan_records(u.t_rec, s0, s1, s_rec, have, [&](const int4& c) { take(me, c); });
        }
        if (have) done(me, u.q_row0 + me.z);
    }
}

// grid (N * nb).  R = isqrt(max radius2), box = min(R, max(H, W)): the reach in pixels that picks the bucket range.
template <bool SELF>
__global__ __launch_bounds__(kThreads) void spatial_within_kernel(PointSet q, PointSet t, Grid g, Cells qc, Cells tc, Radii radii, int n_r, int R,
                                                                  int box, int32_t* __restrict__ counts,
                                                                  unsigned long long* __restrict__ pair_counts) {
    __shared__ int4 s_rec[kChunk];
    __shared__ long long s_sum[kThreads / 64];
    Query u;
    if (!open_query(q, t, g, qc, tc, u)) return;
    long long sum[kMaxRadii];
#pragma unroll
    for (int j = 0; j < kMaxRadii; ++j) sum[j] = 0;
    int cnt[kMaxRadii];
    walk_box(
        u, g, box, s_rec,
        [&](const int4&) {
#pragma unroll
            for (int j = 0; j < kMaxRadii; ++j) cnt[j] = 0;
        },
        [&](const int4& me, const int4& c) {
            if (SELF && c.z == me.z) return;
            const int dr = c.x - me.x, dc = c.y - me.y;
            if (dr > R || dr < -R || dc > R || dc < -R) return;
            const int d2 = dr * dr + dc * dc;
#pragma unroll
            for (int j = 0; j < kMaxRadii; ++j) cnt[j] += (j < n_r && d2 <= radii.r2[j]) ? 1 : 0;
        },
        [&](const int4&, long long row) {
#pragma unroll
            for (int j = 0; j < kMaxRadii; ++j)
                if (j < n_r) {
                    counts[row * n_r + j] = cnt[j];
                    sum[j] += cnt[j];
                }
        });
    const int n = blockIdx.x / g.nb;
#pragma unroll
    for (int j = 0; j < kMaxRadii; ++j)
        if (j < n_r) {                                                     // n_r is uniform: every thread reaches the barriers
            const long long all = block_reduce<kThreads, long long>(sum[j], [](long long a, long long c) { return a + c; }, s_sum);
            if (threadIdx.x == 0 && all) atomicAdd(pair_counts + (long long)n * n_r + j, (unsigned long long)all);
        }
}

// ---- density-based clustering (DBSCAN) of every image's live points -------------------------------------------------------------
// Three box walks at the one radius, then a numbering and a table pass; union-find parents are buffer rows (P < 2^31).
//   core      a point with at least `need` = min_samples - 1 other live points within r2 is a core point; lab[row] = row
//   stamp     one thread per record: the core flag of its point into the record's spare word, so that the next two walks read a
//             candidate's flag from LDS with the candidate
//   unite     every core point with every core neighbour of a lower row: uf_unite hangs the larger root below the smaller, so a
//             cluster's root ends as its smallest core row whatever the order of the unions.  The finds halve their paths
//             (uf_find_halving), a query remembers the root it was last seen under and a candidate is hung straight below the
//             root found for it, so most pairs of a dense clump cost the one load that shows they are united already
//   resolve   lab is only read: root[row] = uf_find for a core point, the smallest root among the core neighbours of another live
//             point, -1 when it has none (noise); the rows that are not live keep the -1 of the fill
//   number    a row with root[row] == row is its cluster's first core point.  G[i] = the number of such rows below i, in two levels:
//             per chunk of 256 rows (block_rank), one workgroup scanning the chunk counts, then chunk base + rank within the chunk.
//             Images are contiguous row ranges and clusters never cross them: cluster id = G[root] - G[off[n]], in the order of the
//             roots, and the image has G[off[n + 1]] - G[off[n]] clusters.
//   table     one thread per row: the label, and integer atomics into row off[n] + id of the tables
// Every value is a count, a minimum or a sum of integers over a set that the definition fixes: nothing depends on the bucket side,
// the launch order or thread timing.  No kernel waits for another workgroup.
constexpr int kCorePass = 0, kUnitePass = 1, kResolvePass = 2;
constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;

struct ClusterWork {
    int32_t* lab;                                  // [P]       union-find parents
    int32_t* root;                                 // [P]       the cluster's smallest core row, -1: none
    int32_t* G;                                    // [P + 1]   cluster roots in the rows below
    int32_t* chunk;                                // [P / 256 + 1]
};
struct ClusterTables {
    int32_t* size;                                 // [P]       row off[n] + c: cluster c of image n
    int32_t* n_core;                               // [P]
    unsigned long long* sums;                      // [P][2] = sum of rows, sum of columns
    int32_t* bbox;                                 // [P][4] = r0, c0, r1, c1 (half-open)
};

// grid (N * nb)
template <int PASS>
__global__ __launch_bounds__(kThreads) void spatial_cluster_walk_kernel(PointSet p, Grid g, Cells cells, int r2, int R, int box, int need,
                                                                        uint8_t* __restrict__ core, ClusterWork w) {
    __shared__ int4 s_rec[kChunk];
    Query u;
    if (!open_query(p, p, g, cells, cells, u)) return;
    // core: the neighbours within r2; unite: the root the query was last seen under; resolve: the smallest root among the core ones
    int acc = 0;
    walk_box(
        u, g, box, s_rec,
        [&](const int4& me) { acc = PASS == kCorePass ? 0 : PASS == kUnitePass ? (int)(u.q_row0 + me.z) : INT_MAX; },
        [&](const int4& me, const int4& c) {
            if (c.z == me.z) return;
            if (PASS != kCorePass && !c.w) return;                         // only core points unite or adopt
            if (PASS == kUnitePass && (!me.w || c.z > me.z)) return;       // every core pair once, from its higher row
            if (PASS == kResolvePass && me.w) return;
            const int dr = c.x - me.x, dc = c.y - me.y;
            if (dr > R || dr < -R || dc > R || dc < -R) return;
            if (dr * dr + dc * dc > r2) return;
            if (PASS == kCorePass) ++acc;
            if (PASS == kUnitePass) {
                // in a dense clump the candidate hangs below the query's root already: one load settles such a pair
                const int up = __hip_atomic_load(w.lab + u.q_row0 + c.z, __ATOMIC_RELAXED, kAgent);
                if (up == acc) return;
                const int a = uf_find_halving<kAgent>(w.lab, acc), b = uf_find_halving<kAgent>(w.lab, up);
                if (b != up) __hip_atomic_fetch_min(w.lab + u.q_row0 + c.z, b, __ATOMIC_RELAXED, kAgent);     // an ancestor, as the halving writes
                if (a != b) uf_unite<kAgent>(w.lab, a, b);
                acc = min(a, b);
            }
            if (PASS == kResolvePass) acc = min(acc, uf_find<kAgent>(w.lab, (int)(u.q_row0 + c.z)));
        },
        [&](const int4& me, long long row) {
            if (PASS == kCorePass) {
                core[row] = acc >= need ? 1 : 0;
                w.lab[row] = (int)row;
            }
            if (PASS == kResolvePass) w.root[row] = me.w ? uf_find<kAgent>(w.lab, (int)row) : (acc == INT_MAX ? -1 : acc);
        });
}

// grid (ceil(P / 256)): slot i of the record buffer belongs to the image whose rows hold it; its first start[n][nb] slots are records
__global__ __launch_bounds__(kThreads) void spatial_cluster_stamp_kernel(PointSet p, Grid g, Cells cells, const uint8_t* __restrict__ core) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int n = i < p.P ? point_image(p, g.N, i) : -1;
    if (n < 0) return;
    const PointWindow w = point_window(p, n);
    const long long slot = i - w.o0;
    if (slot >= w.kept || slot >= cells.start[(long long)n * (g.nb + 1) + g.nb]) return;
    cells.rec[i].w = core[w.o0 + cells.rec[i].z];
}

// grid (P / 256 + 1), rows 0 .. P.  WRITE = false: chunk[block] = the cluster roots among the block's rows.  true, after the scan:
// G[i] = chunk[block] + the roots of the block below i, and the table row i is cleared (lower bounds at INT_MAX: table_kernel lowers
// them, empty_rows_kernel puts the unused rows right).
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void spatial_cluster_rank_kernel(long long P, ClusterWork w, ClusterTables t) {
    __shared__ int s_wsum[kThreads / 64];
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    int total;
    const int before = block_rank<kThreads>(i < P && w.root[i] == i, s_wsum, total);
    if (!WRITE) {
        if (threadIdx.x == 0) w.chunk[blockIdx.x] = total;
        return;
    }
    if (i <= P) w.G[i] = w.chunk[blockIdx.x] + before;
    if (i < P) {
        t.size[i] = 0;
        t.n_core[i] = 0;
        t.sums[2 * i] = 0;
        t.sums[2 * i + 1] = 0;
        t.bbox[4 * i] = INT_MAX;
        t.bbox[4 * i + 1] = INT_MAX;
        t.bbox[4 * i + 2] = 0;
        t.bbox[4 * i + 3] = 0;
    }
}

// grid (1): chunk[0 .. n) -> its exclusive prefix sums, 256 at a time
__global__ __launch_bounds__(kThreads) void spatial_cluster_scan_kernel(int32_t* __restrict__ chunk, int n) {
    __shared__ int s_scan[kThreads];
    int carry = 0;
    for (int j0 = 0; j0 < n; j0 += kThreads) {
        const int j = j0 + threadIdx.x;
        const int v = j < n ? chunk[j] : 0;
        int total;
        const int incl = block_scan_incl<kThreads, int>(v, s_scan, total);
        if (j < n) chunk[j] = carry + incl - v;
        carry += total;
    }
}

constexpr int kTableRounds = 4;

// n points, n_core of them core, with these coordinate sums and bounds (r1, c1 inclusive) into table row `at`
__device__ __forceinline__ void table_add(const ClusterTables& t, long long at, int n, int n_core, int sr, int sc, int r0, int c0, int r1, int c1) {
    atomicAdd(t.size + at, n);
    if (n_core) atomicAdd(t.n_core + at, n_core);
    atomicAdd(t.sums + 2 * at, (unsigned long long)sr);
    atomicAdd(t.sums + 2 * at + 1, (unsigned long long)sc);
    atomicMin(t.bbox + 4 * at, r0);
    atomicMin(t.bbox + 4 * at + 1, c0);
    atomicMax(t.bbox + 4 * at + 2, r1 + 1);
    atomicMax(t.bbox + 4 * at + 3, c1 + 1);
}

// grid (ceil(max(P, N) / 256)): thread i < N writes n_clusters[i], thread i < P the label of row i and its share of the tables
__global__ __launch_bounds__(kThreads) void spatial_cluster_table_kernel(PointSet p, Grid g, ClusterWork w, int32_t* __restrict__ labels,
                                                                         uint8_t* __restrict__ core, int32_t* __restrict__ n_clusters,
                                                                         ClusterTables t) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < g.N) {
        const PointWindow win = point_window(p, (int)i);                   // not ok: o0 = count = 0
        n_clusters[i] = w.G[win.o0 + win.count] - w.G[win.o0];
    }
    Live v = {};
    long long at = -1;                                                     // the table row this thread's point adds to, -1: none
    bool is_core = false;
    if (i < p.P) {
        if (!live_point(p, g, i, v)) {
            labels[i] = -2;
            core[i] = 0;
        } else {
            const int root = w.root[i];
            const int id = root < 0 ? -1 : w.G[root] - w.G[v.o0];
            labels[i] = id;
            if (id >= 0) {
                at = v.o0 + id;
                is_core = core[i] != 0;
            }
        }
    }
    // Lanes of a wave that feed one table row add up first and one of them goes to memory: a slide that is a single aggregate would
    // otherwise queue every point on the same eight addresses.  A few rounds, each for the row of the first lane still waiting; the
    // lanes left after them go on their own.  Sums of integers, minima and maxima: the grouping does not show in the result.
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < kTableRounds; ++round) {
        const unsigned long long waiting = __ballot(at >= 0);
        if (!waiting) break;                                               // uniform over the wave
        const int lead = __builtin_ctzll(waiting);
        const bool in = at >= 0 && at == __shfl(at, lead);
        const unsigned long long group = __ballot(in), cores = __ballot(in && is_core);
        int sr = in ? v.r : 0, sc = in ? v.c : 0, r0 = in ? v.r : INT_MAX, c0 = in ? v.c : INT_MAX, r1 = in ? v.r : -1, c1 = in ? v.c : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off);
            sc += __shfl_xor(sc, off);
            r0 = min(r0, __shfl_xor(r0, off));
            c0 = min(c0, __shfl_xor(c0, off));
            r1 = max(r1, __shfl_xor(r1, off));
            c1 = max(c1, __shfl_xor(c1, off));
        }
        if (lane == lead) table_add(t, at, __popcll(group), __popcll(cores), sr, sc, r0, c0, r1, c1);
        if (in) at = -1;
    }
    if (at >= 0) table_add(t, at, 1, is_core ? 1 : 0, v.r, v.c, v.r, v.c, v.r, v.c);
}

// grid (ceil(P / 256)): the table rows that no cluster owns hold the empty bounding box (0, 0, 0, 0)
__global__ __launch_bounds__(kThreads) void spatial_cluster_empty_rows_kernel(long long P, ClusterTables t) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P || t.size[i] != 0) return;
    t.bbox[4 * i] = 0;
    t.bbox[4 * i + 1] = 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool make_grid(int N, int H, int W, int b, Grid& g) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || b <= 0) return false;
    if ((long long)H * H + (long long)W * W >= (1LL << 31)) return false;
    b = b < (H > W ? H : W) ? b : (H > W ? H : W);                        // a larger side describes the same one-bucket grid
    const long long nbr = (H + (long long)b - 1) / b, nbc = (W + (long long)b - 1) / b;
    if (nbr * nbc * N > kMaxBuckets) return false;
    g = {N, H, W, b, (int)nbr, (int)nbc, (int)(nbr * nbc)};
    return true;
}
size_t cells_bytes(const Grid& g, long long P) {
    return cs_align16((size_t)g.N * g.nb * 4) + cs_align16((size_t)g.N * (g.nb + 1) * 4) + (size_t)(P > 0 ? P : 1) * 16;
}
Cells carve(const Grid& g, long long P, char*& at) {
    Cells c;
    c.cnt = reinterpret_cast<int32_t*>(at);
    at += cs_align16((size_t)g.N * g.nb * 4);
    c.start = reinterpret_cast<int32_t*>(at);
    at += cs_align16((size_t)g.N * (g.nb + 1) * 4);
    c.rec = reinterpret_cast<int4*>(at);
    at += (size_t)(P > 0 ? P : 1) * 16;
    return c;
}
void fill(int32_t* p, long long n, int v, hipStream_t st) {
    if (n <= 0) return;
    const long long blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(spatial_fill_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(kThreads), 0, st, p, n, v);
}
void build(const PointSet& p, const Grid& g, const Cells& c, hipStream_t st) {
    fill(c.cnt, (long long)g.N * g.nb, 0, st);
    const unsigned blocks = (unsigned)((p.P + kThreads - 1) / kThreads);
    if (blocks) hipLaunchKernelGGL(spatial_count_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, p, g, c);
    hipLaunchKernelGGL(spatial_scan_kernel, dim3(g.N), dim3(kThreads), 0, st, g, c);
    if (blocks) hipLaunchKernelGGL(spatial_count_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, p, g, c);
}

// the arguments every query shares: checked, then both grids built
struct Plan {
    Grid g;
    PointSet q, t;
    Cells qc, tc;
    bool self;
};
#define SPATIAL_CHECK_COMMON(name)                                                                                                    \
    Plan plan;                                                                                                                        \
    CS_CHECK_ARG(make_grid(N, H, W, bucket, plan.g), name ": need 0 < N <= 65535, H^2 + W^2 < 2^31, bucket >= 1 and at most 2^22 buckets"); \
    CS_CHECK_ARG(P >= 0 && P < (1LL << 31) && P_other >= 0 && P_other < (1LL << 31), name ": need 0 <= P < 2^31 rows");               \
    CS_CHECK_ARG(off && workspace && (pts || P == 0), name ": NULL argument");                                                        \
    CS_CHECK_ARG(other_off || (!other && !other_limit && P_other == 0), name ": a target set needs its offsets");                    \
    CS_CHECK_ARG(!other_off || other || P_other == 0, name ": NULL argument");                                                        \
    CS_CHECK_ARG((flags & ~1) == 0, name ": unknown flag bits");                                                                      \
    CS_CHECK_ARG(workspace_bytes >= cs_spatial_workspace(N, H, W, bucket, P, other_off ? P_other : -1), name ": workspace too small"); \
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(pts) & 7) == 0 &&                 \
                 (reinterpret_cast<uintptr_t>(other) & 7) == 0 && (reinterpret_cast<uintptr_t>(off) & 7) == 0 &&                      \
                 (reinterpret_cast<uintptr_t>(other_off) & 7) == 0, name ": misaligned argument")

void plan_build(Plan& plan, const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, const int64_t* other,
                const int64_t* other_off, const int32_t* other_limit, long long P_other, int flags, void* workspace, hipStream_t st) {
    char* at = reinterpret_cast<char*>(workspace);
    plan.self = other_off == nullptr;
    plan.q = {pts, off, limit, P, 0};
    plan.qc = carve(plan.g, P, at);
    build(plan.q, plan.g, plan.qc, st);
    if (plan.self) {
        plan.t = plan.q;
        plan.tc = plan.qc;
    } else {
        plan.t = {other, other_off, other_limit, P_other, flags & 1};
        plan.tc = carve(plan.g, P_other, at);
        build(plan.t, plan.g, plan.tc, st);
    }
}

}  // namespace

extern "C" int cs_spatial_threads(void) { return kThreads; }
extern "C" int cs_spatial_chunk(void) { return kChunk; }
extern "C" long long cs_spatial_max_buckets(void) { return kMaxBuckets; }

extern "C" size_t cs_spatial_workspace(int N, int H, int W, int bucket, long long P, long long P_other) {
    Grid g;
    if (!make_grid(N, H, W, bucket, g) || P < 0 || P >= (1LL << 31) || P_other >= (1LL << 31)) return 0;
    return cells_bytes(g, P) + (P_other >= 0 ? cells_bytes(g, P_other) : 0);
}

extern "C" int cs_spatial_nearest(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, const int64_t* other,
                                  const int64_t* other_off, const int32_t* other_limit, long long P_other, int N, int H, int W, int bucket,
                                  int k, int flags, int32_t* index, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream) {
    SPATIAL_CHECK_COMMON("spatial_nearest");
    CS_CHECK_ARG(k >= 1 && k <= kMaxK, "spatial_nearest: need 1 <= k <= 8");
    CS_CHECK_ARG((index && d2) || P == 0, "spatial_nearest: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(index) & 3) == 0 && (reinterpret_cast<uintptr_t>(d2) & 3) == 0, "spatial_nearest: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fill(index, P * k, -2, st);
    fill(d2, P * k, -1, st);
    plan_build(plan, pts, off, limit, P, other, other_off, other_limit, P_other, flags, workspace, st);
    const dim3 grid((unsigned)(plan.g.N * plan.g.nb)), block(kThreads);
#define SPATIAL_NEAREST(KK)                                                                                                              \
    do {                                                                                                                                 \
        if (plan.self) hipLaunchKernelGGL((spatial_nearest_kernel<KK, true>), grid, block, 0, st, plan.q, plan.t, plan.g, plan.qc, plan.tc, k, index, d2); \
        else hipLaunchKernelGGL((spatial_nearest_kernel<KK, false>), grid, block, 0, st, plan.q, plan.t, plan.g, plan.qc, plan.tc, k, index, d2); \
    } while (0)
    if (P > 0) {
        if (k == 1) SPATIAL_NEAREST(1);
        else if (k == 2) SPATIAL_NEAREST(2);
        else if (k <= 4) SPATIAL_NEAREST(4);
        else SPATIAL_NEAREST(8);
    }
#undef SPATIAL_NEAREST
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_spatial_count_within(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, const int64_t* other,
                                       const int64_t* other_off, const int32_t* other_limit, long long P_other, int N, int H, int W,
                                       int bucket, const int32_t* radii2, int n_radii, int flags, int32_t* counts, int64_t* pair_counts,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    SPATIAL_CHECK_COMMON("spatial_count_within");
    CS_CHECK_ARG(radii2 && n_radii >= 1 && n_radii <= kMaxRadii, "spatial_count_within: need 1 to 8 radii");
    Radii radii = {};
    int top = 0;
    for (int j = 0; j < n_radii; ++j) {
        CS_CHECK_ARG(radii2[j] >= 0, "spatial_count_within: radius2 must be non-negative and below 2^31");
        radii.r2[j] = radii2[j];
        top = radii2[j] > top ? radii2[j] : top;
    }
    CS_CHECK_ARG(pair_counts && (counts || P == 0), "spatial_count_within: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(counts) & 3) == 0 && (reinterpret_cast<uintptr_t>(pair_counts) & 7) == 0,
                 "spatial_count_within: misaligned argument");
    int R = 0;                                                            // isqrt(top)
    while ((long long)(R + 1) * (R + 1) <= top) ++R;
    const int box = R < (H > W ? H : W) ? R : (H > W ? H : W);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fill(counts, P * n_radii, -1, st);
    fill(reinterpret_cast<int32_t*>(pair_counts), 2LL * N * n_radii, 0, st);
    plan_build(plan, pts, off, limit, P, other, other_off, other_limit, P_other, flags, workspace, st);
    const dim3 grid((unsigned)(plan.g.N * plan.g.nb)), block(kThreads);
    unsigned long long* pc = reinterpret_cast<unsigned long long*>(pair_counts);
    if (P > 0) {
        if (plan.self) hipLaunchKernelGGL(spatial_within_kernel<true>, grid, block, 0, st, plan.q, plan.t, plan.g, plan.qc, plan.tc, radii, n_radii, R, box, counts, pc);
        else hipLaunchKernelGGL(spatial_within_kernel<false>, grid, block, 0, st, plan.q, plan.t, plan.g, plan.qc, plan.tc, radii, n_radii, R, box, counts, pc);
    }
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" size_t cs_spatial_cluster_workspace(int N, int H, int W, int bucket, long long P) {
    Grid g;
    if (!make_grid(N, H, W, bucket, g) || P < 0 || P >= (1LL << 31)) return 0;
    const size_t rows = (size_t)P;
    return cells_bytes(g, P) + 2 * cs_align16((rows > 0 ? rows : 1) * 4) + cs_align16((rows + 1) * 4) + cs_align16((rows / kThreads + 1) * 4);
}

extern "C" int cs_spatial_cluster(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, int N, int H, int W, int bucket,
                                  int radius2, int min_samples, int32_t* labels, uint8_t* core, int32_t* n_clusters, int32_t* size,
                                  int32_t* n_core, int64_t* sums, int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream) {
    Grid g;
    CS_CHECK_ARG(make_grid(N, H, W, bucket, g), "spatial_cluster: need 0 < N <= 65535, H^2 + W^2 < 2^31, bucket >= 1 and at most 2^22 buckets");
    CS_CHECK_ARG(P >= 0 && P < (1LL << 31), "spatial_cluster: need 0 <= P < 2^31 rows");
    CS_CHECK_ARG(radius2 >= 0, "spatial_cluster: radius2 must be non-negative and below 2^31");
    CS_CHECK_ARG(min_samples >= 1, "spatial_cluster: min_samples must be at least 1");
    CS_CHECK_ARG(off && workspace && n_clusters && (pts || P == 0), "spatial_cluster: NULL argument");
    CS_CHECK_ARG((labels && core && size && n_core && sums && bbox) || P == 0, "spatial_cluster: NULL argument");
    CS_CHECK_ARG(workspace_bytes >= cs_spatial_cluster_workspace(N, H, W, bucket, P), "spatial_cluster: workspace too small");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(pts) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(off) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(n_clusters) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(size) & 3) == 0 && (reinterpret_cast<uintptr_t>(n_core) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(bbox) & 3) == 0, "spatial_cluster: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        fill(n_clusters, N, 0, st);
        CS_LAUNCH_CHECK();
        return CS_OK;
    }
    char* at = reinterpret_cast<char*>(workspace);
    const PointSet p = {pts, off, limit, P, 0};
    const Cells cells = carve(g, P, at);
    ClusterWork w;
    w.lab = reinterpret_cast<int32_t*>(at);
    at += cs_align16((size_t)P * 4);
    w.root = reinterpret_cast<int32_t*>(at);
    at += cs_align16((size_t)P * 4);
    w.G = reinterpret_cast<int32_t*>(at);
    at += cs_align16(((size_t)P + 1) * 4);
    w.chunk = reinterpret_cast<int32_t*>(at);
    const ClusterTables t = {size, n_core, reinterpret_cast<unsigned long long*>(sums), bbox};
    int R = 0;                                                            // isqrt(radius2)
    while ((long long)(R + 1) * (R + 1) <= radius2) ++R;
    const int box = R < (H > W ? H : W) ? R : (H > W ? H : W);
    fill(w.root, P, -1, st);
    build(p, g, cells, st);
    const dim3 walk((unsigned)(g.N * g.nb)), block(kThreads), rows((unsigned)((P + kThreads - 1) / kThreads));
    const unsigned chunks = (unsigned)(P / kThreads + 1);
    const long long most = P > N ? P : N;
    hipLaunchKernelGGL(spatial_cluster_walk_kernel<kCorePass>, walk, block, 0, st, p, g, cells, radius2, R, box, min_samples - 1, core, w);
    hipLaunchKernelGGL(spatial_cluster_stamp_kernel, rows, block, 0, st, p, g, cells, core);
    hipLaunchKernelGGL(spatial_cluster_walk_kernel<kUnitePass>, walk, block, 0, st, p, g, cells, radius2, R, box, 0, core, w);
    hipLaunchKernelGGL(spatial_cluster_walk_kernel<kResolvePass>, walk, block, 0, st, p, g, cells, radius2, R, box, 0, core, w);
    hipLaunchKernelGGL(spatial_cluster_rank_kernel<false>, dim3(chunks), block, 0, st, P, w, t);
    hipLaunchKernelGGL(spatial_cluster_scan_kernel, dim3(1), block, 0, st, w.chunk, (int)chunks);
    hipLaunchKernelGGL(spatial_cluster_rank_kernel<true>, dim3(chunks), block, 0, st, P, w, t);
    hipLaunchKernelGGL(spatial_cluster_table_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads)), block, 0, st, p, g, w, labels, core,
                       n_clusters, t);
    hipLaunchKernelGGL(spatial_cluster_empty_rows_kernel, rows, block, 0, st, P, t);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

extern "C" int cs_spatial_bin_counts(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, int N, int H, int W, int bin,
                                     int32_t* out, void* stream) {
    Grid g;
    CS_CHECK_ARG(make_grid(N, H, W, bin, g), "spatial_bin_counts: need 0 < N <= 65535, H^2 + W^2 < 2^31, bin >= 1 and at most 2^22 bins");
    CS_CHECK_ARG(P >= 0 && P < (1LL << 31), "spatial_bin_counts: need 0 <= P < 2^31 rows");
    CS_CHECK_ARG(off && out && (pts || P == 0), "spatial_bin_counts: NULL argument");
    CS_CHECK_ARG((reinterpret_cast<uintptr_t>(pts) & 7) == 0 && (reinterpret_cast<uintptr_t>(off) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(out) & 3) == 0, "spatial_bin_counts: misaligned argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PointSet p = {pts, off, limit, P, 0};
    const Cells c = {out, nullptr, nullptr};
    fill(out, (long long)N * g.nb, 0, st);
    const unsigned blocks = (unsigned)((P + kThreads - 1) / kThreads);
    if (blocks) hipLaunchKernelGGL(spatial_count_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, p, g, c);
    CS_LAUNCH_CHECK();
    return CS_OK;
}
