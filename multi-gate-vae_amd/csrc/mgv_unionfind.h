// A concurrent union-find over one int32 parent[N] (N < 2^31), shared by csrc/components.hip (pairs from a list) and the tile walk of
// csrc/pair_scores.hip (k_sim_union).
//
// INVARIANT: 0 <= parent[x] <= x at all times, and an entry only ever decreases.  Three writers exist:
//   mgv_cc_init    parent[x] = x                                                       (a kernel of its own, before every hook)
//   hook           compare-and-swap parent[hi] : hi -> lo with lo < hi, i.e. only a ROOT is hooked, and only under a smaller id
//   path halving   fetch_min(parent[x], g) with g the grandparent just read, on a NON-root x (a non-root never becomes a root again)
// x, parent[x] and everything a find passes belong to one tree, and trees only ever merge.  A tree's root is therefore its smallest id,
// whatever the schedule: the final labels are the same bits from run to run.
//
// VISIBILITY: the per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so in a kernel
// that runs while hooks happen EVERY access to parent is an agent-scope atomic (relaxed load, compare-exchange, fetch_min) — no plain
// load or store.  A plain load that kept returning a stale "I am a root" would make a hook retry for ever.  Kernels separated from the
// hooks by a kernel boundary (init, labels) use plain accesses.
//
// TERMINATION:
//   find   walks strictly decreasing ids (every step checks 0 <= parent[x] < x, else it is a root or the forest is broken): at most x steps.
//   unite  retries only when its compare-and-swap found parent[hi] != hi, i.e. when ANOTHER hook on hi succeeded in between.  At most N - 1
//          hooks can succeed in all, and after a failure both ends are found again from where they were, so max(ra, rb) has decreased:
//          no schedule makes a thread retry more than 2 N times.  No thread ever waits for another one.
//   cap    every loop nevertheless counts its rounds and gives up at kUfCap: the thread leaves an error record in status and returns,
//          so a broken forest (a parent array that never went through mgv_cc_init) cannot outlive its launch.
#pragma once
#include "mgv_common.h"

namespace mgv {

constexpr int kUfCap = 1 << 20;
constexpr int kUfErrForest = 1;       // status = {1, x, parent[x], steps}: an entry outside [0, x] (not initialised?)
constexpr int kUfErrRounds = 2;       // status = {2, a, b, rounds}: a find or a unite reached kUfCap
constexpr int kUfErrId = 3;           // status = {3, a, b, 0}: a listed id outside [0, N); the pair was skipped

// the first error wins; the record is read by the host after the kernel (plain vector stores are enough for the payload)
__device__ inline void uf_fail(int32_t* status, int code, int a, int b, int rounds) {
    int expected = 0;
    if (__hip_atomic_compare_exchange_strong(status, &expected, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        status[1] = a; status[2] = b; status[3] = rounds;
    }
}

__device__ __forceinline__ int uf_load(const int32_t* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x at some moment of the call, or -1 after an error record.  Strictly decreasing ids (see TERMINATION); path halving.
__device__ inline int uf_find(int32_t* parent, int x, int32_t* status) {
    for (int steps = 0; steps < kUfCap; ++steps) {
        const int p = uf_load(parent, x);
        if (p == x) return x;
        if (p < 0 || p > x) { uf_fail(status, kUfErrForest, x, p, steps); return -1; }
        const int g = uf_load(parent, p);
        if (g == p) return p;
        if (g < 0 || g > p) { uf_fail(status, kUfErrForest, p, g, steps); return -1; }
        __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // g < p < x: the entry decreases
        x = g;
    }
    uf_fail(status, kUfErrRounds, x, x, kUfCap);
    return -1;
}

// one tree for a and b (0 <= a, b < N).  Pairs whose roots already agree cost two finds and no write.
__device__ inline void uf_unite(int32_t* parent, int a, int b, int32_t* status) {
    int ra = uf_find(parent, a, status), rb = uf_find(parent, b, status);
    for (int rounds = 0; ra >= 0 && rb >= 0 && ra != rb; ++rounds) {
        if (rounds >= kUfCap) { uf_fail(status, kUfErrRounds, a, b, rounds); return; }
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;                                        // hi was still a root: hooked under the smaller root
        ra = uf_find(parent, hi, status);                  // another hook took hi: both ends again, from where they were
        rb = uf_find(parent, lo, status);
    }
}

}  // namespace mgv
