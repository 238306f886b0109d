// Workgroup-level primitives of the post-processing kernels (topk.hip, detect.hip, regions.hip): device-only, stateless, integer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Inclusive prefix sum of v over the NT threads of the workgroup (Hillis-Steele in LDS); V is int or long long.
// Contract: EVERY thread of the workgroup calls it (it holds barriers), with `scratch` = NT elements of LDS owned by the caller.
// On return every thread holds its inclusive value and, in `total`, the sum over the workgroup, and `scratch` may be written
// again at once: the last barrier below is the one that makes this true.  Both loops of this file stay rolled: unrolled, their
// hoisted LDS addresses / loaded words cost 8 to 19 VGPRs per call site, and the barriers, not the loop control, set the time.
template <int NT, typename V>
__device__ __forceinline__ V block_scan_incl(V v, V* scratch, V& total) {
    const int t = threadIdx.x;
    scratch[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < NT; off <<= 1) {
        const V add = t >= off ? scratch[t - off] : 0;
        __syncthreads();
        scratch[t] += add;
        __syncthreads();
    }
    const V incl = scratch[t];
    total = scratch[NT - 1];
    __syncthreads();
    return incl;
}

// Number of threads of the workgroup with a lower index whose flag is set; `total` = number of set flags in the workgroup.
// Contract: EVERY thread of the NT-thread workgroup calls it (ballot and barriers), with `wsum` = NT / 64 ints of LDS owned by the
// caller; `wsum` may be written again on return.
template <int NT>
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll 1
    for (int w = 0; w < NT / 64; ++w) {
        const int s = wsum[w];
        before += w < wv ? s : 0;
        all += s;
    }
    total = all;
    __syncthreads();
    return before;
}

// Lock-free union-find over labels that only ever decrease (lab[x] <= x, a root has lab[x] == x); relaxed atomics at SCOPE =
// __HIP_MEMORY_SCOPE_WORKGROUP (labels in LDS) or __HIP_MEMORY_SCOPE_AGENT (global memory).  Nothing waits on another thread.
template <int SCOPE>
__device__ __forceinline__ int uf_find(const int32_t* lab, int x) {
    int q;
    while ((q = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, SCOPE)) != x) x = q;
    return x;
}
// uf_find that halves the path it walks: every label on it is lowered to its grandparent, with an atomic minimum, so a label still
// only decreases and still names a member of its own set, and a root is never written.  Concurrent uf_unite / uf_find stay
// correct; the forest is the same partition with shorter paths.  For passes that may write the labels.
template <int SCOPE>
__device__ __forceinline__ int uf_find_halving(int32_t* lab, int x) {
    for (;;) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        const int g = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, SCOPE);
        if (g == p) return p;
        __hip_atomic_fetch_min(lab + x, g, __ATOMIC_RELAXED, SCOPE);
        x = g;
    }
}
// Hangs the larger root below the smaller.  Every turn that does not end the loop lowers max(a, b): bounded by the index range.
template <int SCOPE>
__device__ __forceinline__ void uf_unite(int32_t* lab, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(lab, a);
        b = uf_find<SCOPE>(lab, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = __hip_atomic_fetch_min(lab + hi, lo, __ATOMIC_RELAXED, SCOPE);
        if (old == hi) return;         // hi was a root and now hangs below lo
        a = old;                       // hi had a parent already: that parent and lo are still to be united
        b = lo;
    }
}

// op(., .) folded over the values v of the NT threads of the workgroup: xor shuffles within a wave, one slot of LDS per wave
// across; op is associative and commutative, V a type the shuffles move (int, long long).  Contract: EVERY thread of the
// workgroup calls it (it holds barriers), with `slots` = NT / 64 elements of LDS owned by the caller; every thread gets the
// result and `slots` may be written again on return.
template <int NT, typename V, typename Op>
__device__ __forceinline__ V block_reduce(V v, Op op, V* slots) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    V all = slots[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) all = op(all, slots[w]);
    __syncthreads();
    return all;
}
