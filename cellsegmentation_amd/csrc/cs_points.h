// The ragged point set of the post-processing kernels (score.hip, spatial.hip, regions.hip's splits, render.hip's points): pts int64
// [P][2], off int64 [N + 1], limit int32 [N] or NULL, as cs_detect_cluster leaves them.  Image n owns rows off[n] .. off[n + 1] of the
// buffer, which may hold spare rows after off[N]; limit[n] = c keeps the rows Python's [:c] keeps.  An image whose offsets do not
// describe rows of the buffer has no rows at all, and no offsets array makes anything here read outside off[0 .. N] or limit[0 .. N).
// What a consumer does with a kept row -- inside the image or not, (row, col) or (col, row) by `xy` -- is its own business.
//
// Plain C++ without device intrinsics: tests/host/points_window.cpp compiles it for the host and compares it with a slice.
#pragma once
#include <limits.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CS_POINTS_FN __host__ __device__ __forceinline__
#else
#define CS_POINTS_FN inline
#endif

struct PointSet {
    const int64_t* pts;                            // [P][2]
    const int64_t* off;                            // [N + 1]
    const int32_t* limit;                          // [N] or NULL
    long long P;                                   // rows of the buffer
    int xy;                                        // 1: the rows are (col, row)
};

// rows [o0, o0 + count) of the buffer are image n's, the first `kept` of them within its limit; !ok: the offsets do not describe
// rows of a buffer of P rows, and o0 = count = kept = 0
struct PointWindow {
    long long o0;
    int count, kept;
    bool ok;
};
CS_POINTS_FN PointWindow point_window(long long o0, long long o1, long long P, const int32_t* limit, int n) {
    const bool ok = o0 >= 0 && o1 >= o0 && o1 <= P && o1 - o0 <= INT_MAX;
    const int count = ok ? (int)(o1 - o0) : 0;
    const int c = limit ? limit[n] : count;        // Python's [:c]
    const int kept = c >= 0 ? (c < count ? c : count) : (count + c > 0 ? count + c : 0);
    return {ok ? o0 : 0, count, kept, ok};
}
CS_POINTS_FN PointWindow point_window(const PointSet& s, int n) { return point_window(s.off[n], s.off[n + 1], s.P, s.limit, n); }

// the image whose rows hold row i of the buffer -- the last n in [0, N) with off[n] <= i, where off[n + 1] > i -- or -1
CS_POINTS_FN int point_image(const PointSet& s, int N, long long i) {
    if (s.off[0] > i) return -1;
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return s.off[hi] <= i ? -1 : lo;               // beyond the last image
}
