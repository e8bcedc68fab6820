// lbfgspp_amd/csrc/graph_topology.hip -- the incidence list of a graph objective, built on the device at bind
// (include/lbfgsx.h, "graph objectives"; walked by graph_kernels.cuh).
//
//   1. the caller's ei[E], ej[E] (host or device) are copied into buffers of this call;
//   2. k_graph_validate reduces the count of offending edges (an index outside [0, n), or ei[e] == ej[e]) and the smallest
//      offending e; any offender ends the build with LBFGSX_E_INVALID and leaves the context without a list, so that no
//      evaluation kernel ever runs on an index that was not checked;
//   3. the 2E (node, (e << 1) | side) pairs, in the order e = 0 side 0, e = 0 side 1, e = 1 side 0, .., are sorted by node
//      with rocprim::radix_sort_pairs, which is stable: within a node the entries stay in ascending e;
//   4. off[v] = the first sorted position whose node is >= v (a binary search per node, v = 0 .. n), entries are written as
//      {other end, (e << 1) | side}.
// The list belongs to the context and is rebuilt at every bind; nothing is cached by pointer.
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <string>
#include <vector>

#include "graph_entry.hpp"
#include "launch_args.hpp"

namespace lbfgsx {
namespace {

constexpr unsigned long long kNoEdge = ~0ull;

// res[0] += offending edges, res[1] = min(res[1], smallest offending e)
__global__ void __launch_bounds__(kBlock) k_graph_validate(const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                           int64_t E, int64_t n, unsigned long long* __restrict__ res)
{
    unsigned long long cnt = 0, first = kNoEdge;
    for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < E; e += int64_t(gridDim.x) * kBlock)
    {
        const int64_t i = ei[e], j = ej[e];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j)
        {
            cnt++;
            if (first == kNoEdge)
                first = (unsigned long long) e;
        }
    }
    if (cnt)
    {
        atomicAdd(&res[0], cnt);
        atomicMin(&res[1], first);
    }
}

__global__ void __launch_bounds__(kBlock) k_graph_expand(const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                         int64_t E, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < E; e += int64_t(gridDim.x) * kBlock)
    {
        keys[2 * e] = uint32_t(ei[e]);
        keys[2 * e + 1] = uint32_t(ej[e]);
        vals[2 * e] = uint32_t(e) << 1;
        vals[2 * e + 1] = (uint32_t(e) << 1) | 1u;
    }
}

// off[v] = the number of sorted keys below v, v = 0 .. n
__global__ void __launch_bounds__(kBlock) k_graph_offsets(const uint32_t* __restrict__ keys, int64_t m, int64_t n,
                                                          uint32_t* __restrict__ off)
{
    for (int64_t v = int64_t(blockIdx.x) * kBlock + threadIdx.x; v <= n; v += int64_t(gridDim.x) * kBlock)
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

__global__ void __launch_bounds__(kBlock) k_graph_entries(const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                          const uint32_t* __restrict__ vals, int64_t m,
                                                          GraphEntry* __restrict__ inc)
{
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < m; q += int64_t(gridDim.x) * kBlock)
    {
        const uint32_t es = vals[q];
        const int64_t e = es >> 1;
        GraphEntry en;
        en.other = (es & 1u) ? ei[e] : ej[e];
        en.es = es;
        inc[q] = en;
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

void graph_topology_free(lbfgsx_ctx* c)
{
    (void) hipFree(c->graph_off);
    (void) hipFree(c->graph_inc);
    c->graph_off = c->graph_inc = nullptr;
    c->graph_E = 0;
    c->mesh_K = c->mesh_D = 0;
    linear_topology_free(c);
    dense_topology_free(c);
}

int graph_topology_build(lbfgsx_ctx* c, const int32_t* ei, const int32_t* ej, int64_t E, int on_device)
{
    LBFGSX_HIP(stream_sync(c->stream));  // no launch of an earlier binding still walks the list this call frees
    graph_topology_free(c);
    const int64_t n = c->n, m = 2 * E;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    Temps t;
    int32_t *dei = nullptr, *dej = nullptr;
    unsigned long long* res = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&dei), size_t(E) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&dej), size_t(E) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&res), 16));
    const unsigned long long init[2] = {0, kNoEdge};
    unsigned long long got[2] = {0, kNoEdge};
    LBFGSX_HIP(copy_async(dei, ei, size_t(E) * 4, kind, c->stream));
    LBFGSX_HIP(copy_async(dej, ej, size_t(E) * 4, kind, c->stream));
    LBFGSX_HIP(copy_async(res, init, 16, hipMemcpyHostToDevice, c->stream));
    LBFGSX_LAUNCH(k_graph_validate, dim3(grid_of(E)), dim3(kBlock), 0, c->stream, dei, dej, E, n, res);
    LBFGSX_HIP(copy_async(got, res, 16, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    if (got[0])
    {
        int32_t bi = 0, bj = 0;
        LBFGSX_HIP(copy_async(&bi, dei + got[1], 4, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(copy_async(&bj, dej + got[1], 4, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(stream_sync(c->stream));
        set_error("graph objective: edge e = " + std::to_string(got[1]) + " is (i = " + std::to_string(bi) + ", j = " +
                  std::to_string(bj) + ") with n = " + std::to_string(n) + ": an edge joins two different nodes in [0, n); " +
                  std::to_string(got[0]) + " of the E = " + std::to_string(E) + " edges offend, this is the first");
        return LBFGSX_E_INVALID;
    }
    uint32_t *kin = nullptr, *kout = nullptr, *vin = nullptr, *vout = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kin), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kout), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&vin), size_t(m) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&vout), size_t(m) * 4));
    LBFGSX_LAUNCH(k_graph_expand, dim3(grid_of(E)), dim3(kBlock), 0, c->stream, dei, dej, E, kin, vin);
    unsigned end_bit = 1;
    while (end_bit < 32 && (uint64_t(n - 1) >> end_bit) != 0)
        end_bit++;
    size_t bytes = 0;
    void* tmp = nullptr;
    LBFGSX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, size_t(m), 0, end_bit, c->stream));
    LBFGSX_HIP(t.get(&tmp, bytes));
    counters().launches.fetch_add(1, std::memory_order_relaxed);
    LBFGSX_HIP(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, size_t(m), 0, end_bit, c->stream));
    void *off = nullptr, *inc = nullptr;
    LBFGSX_HIP(hipMalloc(&off, size_t(n + 1) * 4));
    if (hipMalloc(&inc, size_t(m) * sizeof(GraphEntry)) != hipSuccess)
    {
        (void) hipFree(off);
        set_error("graph objective: no device memory for the incidence list of E = " + std::to_string(E) + " edges");
        return LBFGSX_E_HIP;
    }
    c->graph_off = off;
    c->graph_inc = inc;
    c->graph_E = E;
    LBFGSX_LAUNCH(k_graph_offsets, dim3(grid_of(n + 1)), dim3(kBlock), 0, c->stream, kout, m, n, static_cast<uint32_t*>(off));
    LBFGSX_LAUNCH(k_graph_entries, dim3(grid_of(m)), dim3(kBlock), 0, c->stream, dei, dej, vout, m,
                  static_cast<GraphEntry*>(inc));
    const hipError_t e = stream_sync(c->stream);  // the temporaries go when this returns
    if (e != hipSuccess)
    {
        graph_topology_free(c);
        set_error(std::string("graph objective: building the incidence list failed: ") + hipGetErrorString(e));
        return LBFGSX_E_HIP;
    }
    return LBFGSX_OK;
}

int graph_topology_read(lbfgsx_ctx* c, uint32_t* off, int32_t* other, uint32_t* edge_side)
{
    const int64_t m = 2 * c->graph_E;
    if (off)
        LBFGSX_HIP(copy_async(off, c->graph_off, size_t(c->n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<GraphEntry> h;
    if (other || edge_side)
    {
        h.resize(size_t(m));
        LBFGSX_HIP(copy_async(h.data(), c->graph_inc, size_t(m) * sizeof(GraphEntry), hipMemcpyDeviceToHost, c->stream));
    }
    LBFGSX_HIP(stream_sync(c->stream));
    for (int64_t q = 0; q < int64_t(h.size()); q++)
    {
        if (other)
            other[q] = h[size_t(q)].other;
        if (edge_side)
            edge_side[q] = h[size_t(q)].es;
    }
    return LBFGSX_OK;
}

}  // namespace lbfgsx
