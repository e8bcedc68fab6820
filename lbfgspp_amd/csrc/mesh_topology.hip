// lbfgspp_amd/csrc/mesh_topology.hip -- the incidence list of a mesh objective, built on the device at bind
// (include/lbfgsx.h, "mesh objectives"; walked by mesh_kernels.cuh).  The steps of graph_topology.hip, in its order:
//   1. the caller's elems[E*K] (host or device, K node indices per element) is copied into a buffer of this call;
//   2. k_mesh_validate, which reads only that table, reduces the count of offending elements (an index outside [0, N), or
//      two equal indices in one element) and the smallest offending e; any offender ends the build with LBFGSX_E_INVALID and
//      leaves the context without a list: no evaluation kernel ever runs on an index that was not checked;
//   3. the K*E (node, (e << 2) | slot) pairs, e ascending then slot ascending, are sorted by node with the stable
//      rocprim::radix_sort_pairs: within a node the entries stay in ascending e;
//   4. off[v] = the first sorted position whose node is >= v (a binary search per node, v = 0 .. N);
//   5. one entry of K 32-bit words per pair: (e << 2) | slot, then the element's other nodes in ascending slot order.
// The list lives in the context's graph_off, graph_inc, graph_E (a context has one bound objective, so one list) with mesh_K,
// mesh_D, and is rebuilt at every bind; nothing is cached by pointer.
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <string>
#include <vector>

#include "launch_args.hpp"

namespace lbfgsx {
namespace {

constexpr unsigned long long kNoElem = ~0ull;

// res[0] += offending elements, res[1] = min(res[1], smallest offending e)
template <int K>
__global__ void __launch_bounds__(kBlock) k_mesh_validate(const int32_t* __restrict__ el, int64_t E, int64_t N,
                                                          unsigned long long* __restrict__ res)
{
    unsigned long long cnt = 0, first = kNoElem;
    for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < E; e += int64_t(gridDim.x) * kBlock)
    {
        int64_t v[K];
#pragma unroll
        for (int k = 0; k < K; k++)
            v[k] = el[e * K + k];
        bool bad = false;
#pragma unroll
        for (int k = 0; k < K; k++)
        {
            bad = bad || v[k] < 0 || v[k] >= N;
#pragma unroll
            for (int j = 0; j < k; j++)
                bad = bad || v[j] == v[k];
        }
        if (bad)
        {
            cnt++;
            if (first == kNoElem)
                first = (unsigned long long) e;
        }
    }
    if (cnt)
    {
        atomicAdd(&res[0], cnt);
        atomicMin(&res[1], first);
    }
}

// position K*e + slot: key = the node, value = (e << 2) | slot
__global__ void __launch_bounds__(kBlock) k_mesh_expand(const int32_t* __restrict__ el, int64_t m, int K,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < m; q += int64_t(gridDim.x) * kBlock)
    {
        keys[q] = uint32_t(el[q]);
        vals[q] = (uint32_t(q / K) << 2) | uint32_t(q % K);
    }
}

// off[v] = the number of sorted keys below v, v = 0 .. N
__global__ void __launch_bounds__(kBlock) k_mesh_offsets(const uint32_t* __restrict__ keys, int64_t m, int64_t N,
                                                         uint32_t* __restrict__ off)
{
    for (int64_t v = int64_t(blockIdx.x) * kBlock + threadIdx.x; v <= N; v += int64_t(gridDim.x) * kBlock)
    {
        int64_t lo = 0, hi = m;
        while (lo < hi)
        {
            const int64_t mid = lo + (hi - lo) / 2;
            if (int64_t(keys[mid]) < v)
                lo = mid + 1;
            else
                hi = mid;
        }
        off[v] = uint32_t(lo);
    }
}

template <int K>
__global__ void __launch_bounds__(kBlock) k_mesh_entries(const int32_t* __restrict__ el, const uint32_t* __restrict__ vals,
                                                         int64_t m, uint32_t* __restrict__ inc)
{
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < m; q += int64_t(gridDim.x) * kBlock)
    {
        const uint32_t es = vals[q];
        const int64_t e = es >> 2;
        const int slot = int(es & 3u);
        inc[q * K] = es;
#pragma unroll
        for (int k = 1; k < K; k++)  // the (k-1)-th other node: slot k-1 below the own slot, slot k above it
            inc[q * K + k] = uint32_t(el[e * K + (k - 1 < slot ? k - 1 : k)]);
    }
}

// device buffers of one build, freed when it ends
struct Temps
{
    std::vector<void*> p;
    ~Temps()
    {
        for (void* q : p)
            (void) hipFree(q);
    }
    hipError_t get(void** out, size_t bytes)
    {
        const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess)
            p.push_back(*out);
        return e;
    }
};

int grid_of(int64_t items)
{
    int64_t b = (items + kBlock - 1) / kBlock;
    return int(b < 1 ? 1 : (b > kGridCap ? kGridCap : b));
}

}  // namespace

// K in {2, 3, 4}, D in {1, 2, 3}, c->n a multiple of D, 1 <= E <= 2^30 - 1 (lbfgsx_objective_bind_mesh)
int mesh_topology_build(lbfgsx_ctx* c, int K, int D, const int32_t* elems, int64_t E, int on_device)
{
    LBFGSX_HIP(stream_sync(c->stream));  // no launch of an earlier binding still walks the list this call frees
    graph_topology_free(c);
    const int64_t N = c->n / D, m = int64_t(K) * E;
    Temps t;
    int32_t* del = nullptr;
    unsigned long long* res = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&del), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&res), 16));
    const unsigned long long init[2] = {0, kNoElem};
    unsigned long long got[2] = {0, kNoElem};
    LBFGSX_HIP(copy_async(del, elems, size_t(m) * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    LBFGSX_HIP(copy_async(res, init, 16, hipMemcpyHostToDevice, c->stream));
    if (K == 2)
        LBFGSX_LAUNCH(k_mesh_validate<2>, dim3(grid_of(E)), dim3(kBlock), 0, c->stream, del, E, N, res);
    else if (K == 3)
        LBFGSX_LAUNCH(k_mesh_validate<3>, dim3(grid_of(E)), dim3(kBlock), 0, c->stream, del, E, N, res);
    else
        LBFGSX_LAUNCH(k_mesh_validate<4>, dim3(grid_of(E)), dim3(kBlock), 0, c->stream, del, E, N, res);
    LBFGSX_HIP(copy_async(got, res, 16, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    if (got[0])
    {
        int32_t bad[4] = {0, 0, 0, 0};
        LBFGSX_HIP(copy_async(bad, del + got[1] * K, size_t(K) * 4, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(stream_sync(c->stream));
        std::string nodes;
        for (int k = 0; k < K; k++)
            nodes += (k ? ", " : "") + std::to_string(bad[k]);
        set_error("mesh objective: element e = " + std::to_string(got[1]) + " is (" + nodes + ") with N = " + std::to_string(N) +
                  ": an element joins K = " + std::to_string(K) + " different nodes in [0, N); " + std::to_string(got[0]) +
                  " of the E = " + std::to_string(E) + " elements offend, this is the first");
        return LBFGSX_E_INVALID;
    }
    uint32_t *kin = nullptr, *kout = nullptr, *vin = nullptr, *vout = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kin), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kout), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&vin), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&vout), size_t(m) * 4));
    LBFGSX_LAUNCH(k_mesh_expand, dim3(grid_of(m)), dim3(kBlock), 0, c->stream, del, m, K, kin, vin);
    unsigned end_bit = 1;
    while (end_bit < 32 && (uint64_t(N - 1) >> end_bit) != 0)
        end_bit++;
    size_t bytes = 0;
    void* tmp = nullptr;
    LBFGSX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, size_t(m), 0, end_bit, c->stream));
    LBFGSX_HIP(t.get(&tmp, bytes));
    counters().launches.fetch_add(1, std::memory_order_relaxed);
    LBFGSX_HIP(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, size_t(m), 0, end_bit, c->stream));
    void *off = nullptr, *inc = nullptr;
    LBFGSX_HIP(hipMalloc(&off, size_t(N + 1) * 4));
    if (hipMalloc(&inc, size_t(m) * size_t(K) * 4) != hipSuccess)
    {
        (void) hipFree(off);
        set_error("mesh objective: no device memory for the incidence list of E = " + std::to_string(E) + " elements of K = " +
                  std::to_string(K) + " nodes");
        return LBFGSX_E_HIP;
    }
    c->graph_off = off;
    c->graph_inc = inc;
    c->graph_E = E;
    c->mesh_K = K;
    c->mesh_D = D;
    LBFGSX_LAUNCH(k_mesh_offsets, dim3(grid_of(N + 1)), dim3(kBlock), 0, c->stream, kout, m, N, static_cast<uint32_t*>(off));
    if (K == 2)
        LBFGSX_LAUNCH(k_mesh_entries<2>, dim3(grid_of(m)), dim3(kBlock), 0, c->stream, del, vout, m, static_cast<uint32_t*>(inc));
    else if (K == 3)
        LBFGSX_LAUNCH(k_mesh_entries<3>, dim3(grid_of(m)), dim3(kBlock), 0, c->stream, del, vout, m, static_cast<uint32_t*>(inc));
    else
        LBFGSX_LAUNCH(k_mesh_entries<4>, dim3(grid_of(m)), dim3(kBlock), 0, c->stream, del, vout, m, static_cast<uint32_t*>(inc));
    const hipError_t e = stream_sync(c->stream);  // the temporaries go when this returns
    if (e != hipSuccess)
    {
        graph_topology_free(c);
        set_error(std::string("mesh objective: building the incidence list failed: ") + hipGetErrorString(e));
        return LBFGSX_E_HIP;
    }
    return LBFGSX_OK;
}

int mesh_topology_read(lbfgsx_ctx* c, uint32_t* off, uint32_t* words)
{
    const int64_t N = c->n / c->mesh_D, m = int64_t(c->mesh_K) * c->graph_E;
    if (off)
        LBFGSX_HIP(copy_async(off, c->graph_off, size_t(N + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (words)
        LBFGSX_HIP(copy_async(words, c->graph_inc, size_t(m) * size_t(c->mesh_K) * 4, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    return LBFGSX_OK;
}

}  // namespace lbfgsx
