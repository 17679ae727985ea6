// Connected components on the device (added functionality): candidate classes for SAT sweeping from the thresholded cosine relation on
// hf (trainer.py:158-160) and components of decoded link lists (digae_layer.py:31-33).  The union-find itself is mgv_unionfind.h (its
// invariant, visibility rule and termination argument are written there); here are its kernels over a pair list, the final labelling
// with class sizes, and the compact table of the classes with at least min_size members.  Integer work only: every result is exact and
// the same bits from call to call.
#include "mgv_unionfind.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

__global__ __launch_bounds__(kThreads) void k_cc_init(int64_t N, int32_t* parent, int32_t* status) {
    if (blockIdx.x == 0 && threadIdx.x < 4) status[threadIdx.x] = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) parent[i] = (int32_t)i;
}

// one pair per thread, grid-stride; every access to parent inside uf_unite is an agent-scope atomic
__global__ __launch_bounds__(kThreads) void k_cc_union_pairs(int64_t N, int64_t P, const int64_t* a, const int64_t* b, int32_t* parent,
                                                             int32_t* status) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < P; e += (int64_t)gridDim.x * kThreads) {
        const int64_t u = a[e], v = b[e];
        if (u < 0 || u >= N || v < 0 || v >= N) { uf_fail(status, kUfErrId, (int)u, (int)v, 0); continue; }
        if (u != v) uf_unite(parent, (int)u, (int)v, status);
    }
}

// After the hooks (kernel boundary): plain loads.  label[i] = the root of i, size[i] = 0.  An entry outside [0, x) ends the walk (a root,
// or a forest that never was one: nothing outside [0, N) is touched either way).
__global__ __launch_bounds__(kThreads) void k_cc_roots(int64_t N, const int32_t* parent, int32_t* label, int32_t* size) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        int x = (int)i;
        for (;;) {                                         // strictly decreasing ids: at most i steps
            const int p = parent[x];
            if (p < 0 || p >= x) break;
            x = p;
        }
        label[i] = x;
        if (size != nullptr) size[i] = 0;
    }
}

// size[label[i]] += 1 (int32 atomics: exact, order-free); parent (or NULL) is flattened to the labels
__global__ __launch_bounds__(kThreads) void k_cc_sizes(int64_t N, const int32_t* label, int32_t* size, int32_t* parent) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const int r = label[i];
        if (r >= 0 && r < N) atomicAdd(size + r, 1);
        if (parent != nullptr) parent[i] = r;
    }
}

__global__ __launch_bounds__(kThreads) void k_fill_i32(int64_t n, int32_t* x, int32_t v) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) x[i] = v;
}

// root_flag[i]: i is the label of a class of at least min_size; mem_flag[i]: i belongs to one
__global__ __launch_bounds__(kThreads) void k_class_flags(int64_t N, const int32_t* label, const int32_t* size, int min_size,
                                                          int32_t* root_flag, int32_t* mem_flag) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const int r = label[i];
        const bool in = r >= 0 && r < N && size[r] >= min_size;
        mem_flag[i] = in ? 1 : 0;
        root_flag[i] = (in && r == (int)i) ? 1 : 0;
    }
}

// counts = {C, M, status[0..3]}: everything the host reads between sizing and filling
__global__ void k_class_counts(int64_t N, const int32_t* root_pos, const int32_t* mem_pos, const int32_t* status, int32_t* counts) {
    if (threadIdx.x == 0) { counts[0] = root_pos[N]; counts[1] = mem_pos[N]; }
    if (threadIdx.x < 4) counts[2 + threadIdx.x] = status != nullptr ? status[threadIdx.x] : 0;
}

// the selected nodes in ascending id order with their labels as sort keys
__global__ __launch_bounds__(kThreads) void k_class_compact(int64_t N, const int32_t* label, const int32_t* mem_pos, int32_t M,
                                                            uint32_t* keys, int32_t* ids) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const int at = mem_pos[i];
        if (mem_pos[i + 1] != at && at >= 0 && at < M) { keys[at] = (uint32_t)label[i]; ids[at] = (int32_t)i; }
    }
}

// after the stable sort by label: members in (label, id) order; a class starts where the key changes, and its number is the rank of its
// label among the selected roots
__global__ __launch_bounds__(kThreads) void k_class_scatter(int64_t N, int32_t M, int32_t C, const uint32_t* keys_sorted, const int32_t* order,
                                                            const int32_t* ids, const int32_t* root_pos, int64_t* class_ptr,
                                                            int32_t* members) {
    if (blockIdx.x == 0 && threadIdx.x == 0) class_ptr[C] = M;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < M; j += (int64_t)gridDim.x * kThreads) {
        const int o = order[j];
        if (o >= 0 && o < M) members[j] = ids[o];
        const uint32_t k = keys_sorted[j];
        if ((j == 0 || keys_sorted[j - 1] != k) && (int64_t)k < N) {
            const int c = root_pos[k];
            if (c >= 0 && c < C) class_ptr[c] = j;
        }
    }
}

inline int64_t align64(int64_t x) { return (x + 63) / 64 * 64; }

// workspace of the class table in int32 units: size | root_flag | mem_flag | root_pos | mem_pos | scan | keys | keys_sorted | ids | order
struct ClassWs {
    int64_t size, root_flag, mem_flag, root_pos, mem_pos, scan, keys, keys_sorted, ids, order, total;
    explicit ClassWs(int64_t N) {
        const int64_t n = align64(N + 1);
        size = 0; root_flag = n; mem_flag = 2 * n; root_pos = 3 * n; mem_pos = 4 * n;
        scan = 5 * n;
        keys = scan + align64(N / 2048 + 2);
        keys_sorted = keys + n; ids = keys_sorted + n; order = ids + n;
        total = order + n;
    }
};

inline int key_bits(int64_t N) { int b = 1; while (b < 32 && (1LL << b) < N) ++b; return b; }

}  // namespace mgv

#define MGV_CC_GRID(n) dim3(mgv::grid_for(((n) + mgv::kThreads - 1) / mgv::kThreads, 8)), dim3(mgv::kThreads), 0, st
#define MGV_CC_STEP() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return (int)e__; } while (0)

extern "C" int mgv_cc_init(int64_t N, int32_t* parent, int32_t* status, void* stream) {
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL && status != nullptr && (N == 0 || parent != nullptr));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mgv::k_cc_init, MGV_CC_GRID(N), N, parent, status);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_cc_union_pairs(int64_t N, int64_t P, const int64_t* a, const int64_t* b, int32_t* parent, int32_t* status, void* stream) {
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL && P >= 0 && status != nullptr && (N == 0 || parent != nullptr));
    if (P == 0) return MGV_OK;
    MGV_CHECK_ARG(a != nullptr && b != nullptr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mgv::k_cc_union_pairs, MGV_CC_GRID(P), N, P, a, b, parent, status);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_cc_labels(int64_t N, int32_t* parent, int32_t* label, int32_t* size, void* stream) {
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL);
    if (N == 0) return MGV_OK;
    MGV_CHECK_ARG(parent != nullptr && label != nullptr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mgv::k_cc_roots, MGV_CC_GRID(N), N, parent, label, size);
    MGV_CC_STEP();
    if (size != nullptr) hipLaunchKernelGGL(mgv::k_cc_sizes, MGV_CC_GRID(N), N, label, size, parent);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_cc_class_ws_ints(int64_t N) {
    if (N < 0 || N > 0x7fffffffLL) return -1;
    const int64_t t = mgv::ClassWs(N).total;
    return t <= 0x7fffffffLL ? (int)t : -1;
}

extern "C" int mgv_cc_class_count(int64_t N, const int32_t* label, int min_size, const int32_t* status, int32_t* ws, int64_t ws_ints,
                                  int32_t* counts, void* stream) {
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL && min_size >= 1 && counts != nullptr && ws != nullptr && (N == 0 || label != nullptr));
    MGV_CHECK_ARG(((uintptr_t)ws & 255) == 0);
    const mgv::ClassWs w(N);
    MGV_CHECK_ARG(ws_ints >= w.total);
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        hipLaunchKernelGGL(mgv::k_fill_i32, MGV_CC_GRID(N), N, ws + w.size, 0);
        hipLaunchKernelGGL(mgv::k_cc_sizes, MGV_CC_GRID(N), N, label, ws + w.size, (int32_t*)nullptr);
        hipLaunchKernelGGL(mgv::k_class_flags, MGV_CC_GRID(N), N, label, ws + w.size, min_size, ws + w.root_flag, ws + w.mem_flag);
        MGV_CC_STEP();
    }
    int rc = mgv_scan_exclusive_i32(N, ws + w.root_flag, ws + w.root_pos, ws + w.scan, stream);
    if (rc == MGV_OK) rc = mgv_scan_exclusive_i32(N, ws + w.mem_flag, ws + w.mem_pos, ws + w.scan, stream);
    if (rc != MGV_OK) return rc;
    hipLaunchKernelGGL(mgv::k_class_counts, dim3(1), dim3(64), 0, st, N, ws + w.root_pos, ws + w.mem_pos, status, counts);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_cc_class_fill(int64_t N, const int32_t* label, int64_t C, int64_t M, int32_t* ws, int64_t ws_ints, void* sort_temp,
                                 int64_t sort_temp_ints, int64_t* class_ptr, int32_t* members, void* stream) {
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL && C >= 0 && M >= 0 && C <= M && M <= N && class_ptr != nullptr && ws != nullptr);
    MGV_CHECK_ARG(((uintptr_t)ws & 255) == 0 && (M == 0 || (members != nullptr && label != nullptr)));
    const mgv::ClassWs w(N);
    MGV_CHECK_ARG(ws_ints >= w.total);
    hipStream_t st = (hipStream_t)stream;
    if (M > 0) {
        hipLaunchKernelGGL(mgv::k_class_compact, MGV_CC_GRID(N), N, label, ws + w.mem_pos, (int32_t)M, (uint32_t*)(ws + w.keys), ws + w.ids);
        MGV_CC_STEP();
        const int rc = mgv_sort_pairs(4, M, ws + w.keys, ws + w.keys_sorted, ws + w.order, mgv::key_bits(N), sort_temp, sort_temp_ints, stream);
        if (rc != MGV_OK) return rc;
    }
    hipLaunchKernelGGL(mgv::k_class_scatter, MGV_CC_GRID(M), N, (int32_t)M, (int32_t)C, (const uint32_t*)(ws + w.keys_sorted), ws + w.order,
                       ws + w.ids, ws + w.root_pos, class_ptr, members);
    MGV_LAUNCH_RET();
}
