// csrc/cs_points.h on the host against a slice written out element by element: every offsets array with entries in [-1, P + 1] for
// N <= 3 images and P <= 4 rows, the malformed ones included, every limit in [-P - 1, P + 1] and none.  The arrays are heap blocks
// of exactly N + 1 and N entries, so that a sanitizer build sees any read outside off[0 .. N] or limit[0 .. N).  Prints "ok <cases>"
// and returns 0, or the first disagreement and 1.
#include <stdio.h>
#include <vector>
#include "cs_points.h"

static int fail(const char* what, int N, int P, const int64_t* off, int n, int c, long long got, long long want) {
    printf("%s: N=%d P=%d off=[", what, N, P);
    for (int j = 0; j <= N; ++j) printf("%s%lld", j ? " " : "", (long long)off[j]);
    printf("] n=%d limit=%d: got %lld, want %lld\n", n, c, got, want);
    return 1;
}

int main() {
    const int kNoLimit = 99;
    long long cases = 0;
    for (int N = 1; N <= 3; ++N)
        for (int P = 0; P <= 4; ++P) {
            const int span = P + 3;                                        // values -1 .. P + 1
            int total = 1;
            for (int j = 0; j <= N; ++j) total *= span;
            for (int code = 0; code < total; ++code) {
                int64_t* off = new int64_t[N + 1];
                int32_t* lim = new int32_t[N];
                bool rising = true;
                for (int j = 0, v = code; j <= N; ++j, v /= span) {
                    off[j] = v % span - 1;
                    rising = rising && (j == 0 || off[j] >= off[j - 1]);
                }
                for (int n = 0; n < N; ++n)
                    for (int c = -P - 1; c <= P + 2; ++c) {                // P + 2 stands for "no limits"
                        const bool limited = c <= P + 1;
                        for (int j = 0; j < N; ++j) lim[j] = j == n ? c : kNoLimit + j;
                        const PointSet s = {nullptr, off, limited ? lim : nullptr, P, 0};
                        const PointWindow w = point_window(s, n);
                        // the rows of the buffer that image n owns, then Python's [:c] element by element
                        const bool ok = off[n] >= 0 && off[n + 1] >= off[n] && off[n + 1] <= P;
                        std::vector<long long> rows, kept;
                        if (ok)
                            for (long long i = off[n]; i < off[n + 1]; ++i) rows.push_back(i);
                        for (size_t j = 0; j < rows.size(); ++j)
                            if (!limited || (c >= 0 ? (long long)j < c : (long long)j < (long long)rows.size() + c)) kept.push_back(rows[j]);
                        ++cases;
                        if (w.ok != ok) return fail("ok", N, P, off, n, c, w.ok, ok);
                        if (w.count != (int)rows.size()) return fail("count", N, P, off, n, c, w.count, (long long)rows.size());
                        if (w.kept != (int)kept.size()) return fail("kept", N, P, off, n, c, w.kept, (long long)kept.size());
                        if (w.o0 != (rows.empty() ? (ok ? off[n] : 0) : rows[0])) return fail("o0", N, P, off, n, c, w.o0, off[n]);
                        for (size_t j = 0; j < kept.size(); ++j)
                            if (kept[j] != w.o0 + (long long)j) return fail("kept rows", N, P, off, n, c, w.o0 + (long long)j, kept[j]);
                    }
                const PointSet s = {nullptr, off, nullptr, P, 0};
                for (long long i = -1; i <= P + 1; ++i) {
                    const int got = point_image(s, N, i);
                    int want = -1;                                         // rising offsets: the one image with off[n] <= i < off[n + 1]
                    for (int n = 0; n < N; ++n)
                        if (off[n] <= i && i < off[n + 1]) want = want < 0 ? n : want;
                    ++cases;
                    if (rising && got != want) return fail("point_image", N, P, off, (int)i, 0, got, want);
                    // any offsets: an image that is named holds the row between its two offsets
                    if (got >= N || (got >= 0 && !(off[got] <= i && i < off[got + 1]))) return fail("point_image bounds", N, P, off, (int)i, 0, got, want);
                }
                delete[] off;
                delete[] lim;
            }
        }
    // the entry points that know no row count pass the largest one; a count beyond INT_MAX is refused
    const int64_t big[3] = {5, 5 + (long long)INT_MAX, 6 + 2LL * INT_MAX};
    const PointSet b = {nullptr, big, nullptr, LLONG_MAX, 0};
    if (!point_window(b, 0).ok || point_window(b, 0).count != INT_MAX || point_window(b, 1).ok || point_window(b, 1).count != 0) {
        printf("INT_MAX rows\n");
        return 1;
    }
    printf("ok %lld\n", cases);
    return 0;
}
