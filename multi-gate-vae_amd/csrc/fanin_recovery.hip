// Exact gate recovery of a decoded circuit (mgv_fanin_decode's lists, csrc/pair_scores.hip) against the true fan-in sets: the strictest
// reconstruction metric there is — whether the WHOLE fan-in set of a gate came back, under the constraints a netlist has.
// One thread per row v: the distinct ids of idx[v][0 .. K) that are not -1 are the decoded set, each is looked up in the row's true list
// (strictly ascending, so a set) by binary search BY VALUE — an id is compared, never used as an address, so an id outside [0, N) is
// simply a miss.  The rows with a non-empty true list are the gates; per graph they add {gates, exact, hits, true_total,
// decoded_total} to rec.  Integer sums only: a segmented wave reduction over the rows' graphs (rows of one graph follow each other),
// the wave heads of one graph meet through LDS, and the graph's first row in the workgroup issues one 64-bit atomic per non-zero field:
// the same bytes whatever the order.
#include "mgv_launch.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

constexpr int kRecFields = 5;          // gates, exact, hits, true_total, decoded_total
constexpr int kRecMaxK = 32;

__global__ __launch_bounds__(kThreads) void k_fanin_recovery(int64_t N, int K, const int32_t* idx, const int64_t* tru_ptr, int64_t T,
                                                             const int32_t* tru_src, const int32_t* gp, int G, int32_t* n_hit,
                                                             unsigned long long* rec) {
    __shared__ int sg[kThreads];
    __shared__ int sv[kThreads][kRecFields];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int gid = -1;                                          // the row's graph; -1: a row past N or behind the last graph counts nowhere
    int val[kRecFields] = {0, 0, 0, 0, 0};
    if (v < N) {
        if (gp == nullptr) {
            gid = 0;
        } else {
            int a = 0, b = G;
            while (a < b) { const int m = (a + b) >> 1; if ((int64_t)gp[m + 1] <= v) a = m + 1; else b = m; }
            gid = a < G ? a : -1;
        }
        int64_t tb = tru_ptr[v], te = tru_ptr[v + 1];      // inside [0, T] whatever the table holds
        tb = tb < 0 ? 0 : (tb > T ? T : tb);
        te = te < tb ? tb : (te > T ? T : te);
        int hits = 0, dec = 0;
        for (int j = 0; j < K; ++j) {
            const int id = idx[v * K + j];
            if (id == -1) continue;
            bool seen = false;                             // a repeated id is one member of the set
            for (int i = 0; i < j; ++i) seen = seen || idx[v * K + i] == id;
            if (seen) continue;
            ++dec;
            int64_t a = tb, b = te;
            while (a < b) { const int64_t m = (a + b) >> 1; if (tru_src[m] < id) a = m + 1; else b = m; }
            hits += (a < te && tru_src[a] == id) ? 1 : 0;
        }
        if (n_hit != nullptr) n_hit[v] = hits;
        const int nt = (int)(te - tb);                     // < 2^31: the launcher refuses a longer table
        if (nt > 0 && gid >= 0) {
            val[0] = 1; val[1] = (hits == nt && dec == nt) ? 1 : 0; val[2] = hits; val[3] = nt; val[4] = dec;
        }
    }
    // equal graphs are contiguous: after the steps the first lane of a graph's run in the wave holds the run's sums
    for (int d = 1; d < 64; d <<= 1) {
        const int og = __shfl_down(gid, d, 64);
        const bool take = lane + d < 64 && og == gid;
#pragma unroll
        for (int f = 0; f < kRecFields; ++f) { const int o = __shfl_down(val[f], d, 64); val[f] += take ? o : 0; }
    }
    sg[threadIdx.x] = gid;
#pragma unroll
    for (int f = 0; f < kRecFields; ++f) sv[threadIdx.x][f] = val[f];
    __syncthreads();
    const bool head = gid >= 0 && (threadIdx.x == 0 || sg[threadIdx.x - 1] != gid);    // the graph's first row in the workgroup
    if (head) {
        for (int w2 = w + 1; w2 < kThreads / 64 && sg[64 * w2] == gid; ++w2) {          // the runs of the same graph in the waves behind
#pragma unroll
            for (int f = 0; f < kRecFields; ++f) val[f] += sv[64 * w2][f];
        }
#pragma unroll
        for (int f = 0; f < kRecFields; ++f) {
            if (val[f] != 0) atomicAdd(&rec[(int64_t)gid * kRecFields + f], (unsigned long long)val[f]);
        }
    }
}

}  // namespace mgv

extern "C" int mgv_fanin_recovery(int64_t N, int K, const int32_t* idx, const int64_t* tru_ptr, const int32_t* tru_src,
                                  const int32_t* graph_ptr, int G, int32_t* n_hit, int64_t* rec, void* stream) {
    MGV_CHECK_ARG(K >= 1 && K <= mgv::kRecMaxK);
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL / mgv::kRecMaxK);          // node ids and idx offsets are int32 on the host side
    MGV_CHECK_ARG(rec != nullptr && (graph_ptr == nullptr || G >= 0));
    MGV_CHECK_ARG(N == 0 || (idx != nullptr && tru_ptr != nullptr));
    hipStream_t st = (hipStream_t)stream;
    // the ends of both tables in one blocking step: graph_ptr from 0 to N (NULL: one graph), tru_ptr from 0 to T
    int32_t gends[2] = {0, (int32_t)N};
    int64_t tends[2] = {0, 0};
    hipError_t e = hipSuccess;
    if (graph_ptr != nullptr) {
        e = hipMemcpyAsync(&gends[0], graph_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&gends[1], graph_ptr + G, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && N > 0) e = hipMemcpyAsync(&tends[0], tru_ptr, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && N > 0) e = hipMemcpyAsync(&tends[1], tru_ptr + N, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && (graph_ptr != nullptr || N > 0)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    MGV_CHECK_ARG(gends[0] == 0 && (int64_t)gends[1] == N);
    MGV_CHECK_ARG(tends[0] == 0 && tends[1] >= 0 && tends[1] <= 0x7fffffffLL);
    const int64_t T = tends[1];
    MGV_CHECK_ARG(T == 0 || tru_src != nullptr);
    const int64_t rows = G > 1 && graph_ptr != nullptr ? G : 1;
    e = hipMemsetAsync(rec, 0, sizeof(int64_t) * (size_t)rows * mgv::kRecFields, st);
    if (e != hipSuccess) return (int)e;
    if (N == 0) return MGV_OK;
    hipLaunchKernelGGL(mgv::k_fanin_recovery, dim3((unsigned)((N + mgv::kThreads - 1) / mgv::kThreads)), dim3(mgv::kThreads), 0, st, N, K, idx,
                       tru_ptr, T, tru_src, graph_ptr, G, n_hit, reinterpret_cast<unsigned long long*>(rec));
    MGV_LAUNCH_RET();
}
