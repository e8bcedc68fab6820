// lbfgspp_amd/csrc/linear_topology.hip -- the matrix of a linear-model objective, prepared on the device at bind
// (include/lbfgsx.h, "linear-model objectives"; walked by linear_kernels.cuh), and the one kernel of the form that holds no
// caller text, k_lin_long_cols.  A multi-output objective (linear_multi_kernels.cuh) has the same build over the F = n / D
// columns of its matrix (n below is then F), w of R*D elements and D partials per chunk; k_lin_long_cols takes D at run time.
//
//   1. the caller's rowptr[R+1], col[nnz], val[nnz] (host or device) are copied into arrays the context owns;
//   2. k_lin_validate, the only launch of a refused bind, reduces the count of offending positions and the smallest one:
//      rowptr[0] != 0, rowptr[p] < rowptr[p-1], rowptr[R] != nnz (positions 0 .. R), a col[k] outside [0, n) (position
//      R + 1 + k).  It reads nothing through an index it has not checked.  Any offender ends the build with LBFGSX_E_INVALID
//      and leaves the context without a matrix, so that no evaluation kernel ever runs on an index that was not checked;
//   3. the nnz (col[k], k) pairs, in ascending k, are sorted by column with rocprim::radix_sort_pairs, which is stable:
//      within a column the entries stay in ascending CSR position, i.e. ascending row and the caller's order within a row;
//   4. colptr[j] = the first sorted position whose column is >= j (a binary search per column, j = 0 .. n); entry q gets
//      its CSR position tpos[q], its row trow[q] (a binary search in rowptr) and its value tval[q];
//   5. the columns with more than C = kLinearChunk entries are collected, ordered by column on the host (there are at most
//      nnz / (C + 1) of them) and cut into chunks of C consecutive entries: long_col[nlong], long_chunk[nlong + 1] (the
//      first chunk of each long column), chunk[2 * nchunks] (first and past-the-last entry of each chunk).
// The lanes that share a row in the row pass: linear_lanes_rule.  Everything belongs to the context and is rebuilt at every
// bind; nothing is cached by pointer.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <string>
#include <vector>

#include "launch_args.hpp"

namespace lbfgsx {
namespace {

constexpr unsigned long long kNoPos = ~0ull;

// res[0] += offending positions, res[1] = min(res[1], smallest offending position)
__global__ void __launch_bounds__(kBlock) k_lin_validate(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         int64_t R, int64_t nnz, int64_t n, unsigned long long* __restrict__ res)
{
    unsigned long long cnt = 0, first = kNoPos;
    const int64_t total = R + 1 + nnz;
    for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < total; p += int64_t(gridDim.x) * kBlock)
    {
        bool bad;
        if (p <= R)
        {
            const int64_t v = rowptr[p];
            bad = (p == 0 && v != 0) || (p > 0 && v < int64_t(rowptr[p - 1])) || (p == R && v != nnz);
        }
        else
        {
            const int64_t cj = col[p - R - 1];
            bad = cj < 0 || cj >= n;
        }
        if (bad)
        {
            cnt++;
            if (first == kNoPos)
                first = (unsigned long long) p;
        }
    }
    if (cnt)
    {
        atomicAdd(&res[0], cnt);
        atomicMin(&res[1], first);
    }
}

__global__ void __launch_bounds__(kBlock) k_lin_expand(const int32_t* __restrict__ col, int64_t nnz, uint32_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals)
{
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += int64_t(gridDim.x) * kBlock)
    {
        keys[k] = uint32_t(col[k]);
        vals[k] = uint32_t(k);
    }
}

// colptr[j] = the number of sorted keys below j, j = 0 .. n
__global__ void __launch_bounds__(kBlock) k_lin_colptr(const uint32_t* __restrict__ keys, int64_t m, int64_t n,
                                                       uint32_t* __restrict__ colptr)
{
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j <= n; j += int64_t(gridDim.x) * kBlock)
    {
        int64_t lo = 0, hi = m;
        while (lo < hi)
        {
            const int64_t mid = lo + (hi - lo) / 2;
            if (int64_t(keys[mid]) < j)
                lo = mid + 1;
            else
                hi = mid;
        }
        colptr[j] = uint32_t(lo);
    }
}

// entry q of the transposed list: the row of CSR position k = tpos[q] is the last r with rowptr[r] <= k (rowptr is validated:
// non-decreasing, rowptr[0] = 0, rowptr[R] = nnz > k, so 0 <= r < R)
template <class T>
__global__ void __launch_bounds__(kBlock) k_lin_entries(const int32_t* __restrict__ rowptr, const T* __restrict__ val,
                                                        const uint32_t* __restrict__ tpos, int64_t R, int64_t nnz,
                                                        int32_t* __restrict__ trow, T* __restrict__ tval)
{
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < nnz; q += int64_t(gridDim.x) * kBlock)
    {
        const int64_t k = tpos[q];
        int64_t lo = 0, hi = R;  // the first r in [0, R] with rowptr[r] > k
        while (lo < hi)
        {
            const int64_t mid = lo + (hi - lo) / 2;
            if (int64_t(rowptr[mid]) <= k)
                lo = mid + 1;
            else
                hi = mid;
        }
        trow[q] = int32_t(lo - 1);
        tval[q] = val[k];
    }
}

// the columns with more than C entries, in any order: {column, first entry, past-the-last entry}; cap bounds the list
__global__ void __launch_bounds__(kBlock) k_lin_find_long(const uint32_t* __restrict__ colptr, int64_t n, uint32_t C,
                                                          unsigned int cap, unsigned int* __restrict__ count,
                                                          uint32_t* __restrict__ list)
{
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < n; j += int64_t(gridDim.x) * kBlock)
    {
        const uint32_t lo = colptr[j], hi = colptr[j + 1];
        if (hi - lo > C)
        {
            const unsigned int s = atomicAdd(count, 1u);
            if (s < cap)
            {
                list[3 * s] = uint32_t(j);
                list[3 * s + 1] = lo;
                list[3 * s + 2] = hi;
            }
        }
    }
}

// One block per (chunk b of a long column, output c), blockIdx.x = b*D + c (the scalar form has D = 1): thread t sums the
// products tval[q]*w[trow[q]*D + c] of the chunk's entries t, t + kBlock, .. in ascending order, started from its first (+0
// if it has none); then s_t = s_t + s_{t+h} for t < h, h = kBlock/2 .. 1.  part[b*D + c] is thread 0's value.  Every q lies in
// [0, nnz) and every trow[q] in [0, R) by construction of the list.
template <class T>
__global__ void __launch_bounds__(kBlock) k_lin_long_cols(const uint32_t* __restrict__ chunk, const int32_t* __restrict__ trow,
                                                          const T* __restrict__ tval, const T* __restrict__ w,
                                                          T* __restrict__ part, int D)
{
    __shared__ T sh[kBlock];
    const unsigned b = blockIdx.x / unsigned(D), c = blockIdx.x % unsigned(D);
    const uint32_t beg = chunk[2 * b], end = chunk[2 * b + 1];
    T s = T(0);
    bool has = false;
    for (int64_t q = int64_t(beg) + threadIdx.x; q < int64_t(end); q += kBlock)
    {
        const T prod = tval[q] * w[int64_t(trow[q]) * D + c];
        s = has ? s + prod : prod;
        has = true;
    }
    sh[threadIdx.x] = s;
    for (int h = kBlock / 2; h >= 1; h >>= 1)
    {
        __syncthreads();
        if (int(threadIdx.x) < h)
            sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
    }
    if (threadIdx.x == 0)
        part[blockIdx.x] = sh[0];
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

// an array the context keeps; the caller frees the whole matrix when one allocation fails
hipError_t own(void** out, size_t bytes) { return hipMalloc(out, bytes ? bytes : 1); }

int build(lbfgsx_ctx* c, int64_t R, int64_t nnz, const int32_t* rowptr, const int32_t* col, const void* val, int on_device,
          int lanes, int D)
{
    lbfgsx_ctx::LinearTopo& l = c->lin;
    const int64_t n = D ? c->n / D : c->n;  // the matrix's columns
    const size_t Dw = size_t(D ? D : 1);    // the elements of w per row and of part per chunk
    const std::string name = D ? "multi-output linear-model objective: " : "linear-model objective: ";
    const size_t esz = size_t(c->esz);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    Temps t;
    LBFGSX_HIP(own(&l.rowptr, size_t(R + 1) * 4));
    LBFGSX_HIP(own(&l.col, size_t(nnz) * 4));
    LBFGSX_HIP(own(&l.val, size_t(nnz) * esz));
    unsigned long long* res = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&res), 16));
    const unsigned long long init[2] = {0, kNoPos};
    unsigned long long got[2] = {0, kNoPos};
    LBFGSX_HIP(copy_async(l.rowptr, rowptr, size_t(R + 1) * 4, kind, c->stream));
    LBFGSX_HIP(copy_async(l.col, col, size_t(nnz) * 4, kind, c->stream));
    LBFGSX_HIP(copy_async(l.val, val, size_t(nnz) * esz, kind, c->stream));
    LBFGSX_HIP(copy_async(res, init, 16, hipMemcpyHostToDevice, c->stream));
    const int32_t* drow = static_cast<const int32_t*>(l.rowptr);
    const int32_t* dcol = static_cast<const int32_t*>(l.col);
    LBFGSX_LAUNCH(k_lin_validate, dim3(grid_of(R + 1 + nnz)), dim3(kBlock), 0, c->stream, drow, dcol, R, nnz, n, res);
    LBFGSX_HIP(copy_async(got, res, 16, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    if (got[0])
    {
        const int64_t p = int64_t(got[1]);
        int32_t v = 0;
        const int32_t* src = p <= R ? drow + p : dcol + (p - R - 1);
        LBFGSX_HIP(copy_async(&v, src, 4, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(stream_sync(c->stream));
        std::string what;
        if (p <= R)
            what = "rowptr[" + std::to_string(p) + "] = " + std::to_string(v) + " with R = " + std::to_string(R) + ", nnz = " +
                   std::to_string(nnz) + ": rowptr starts at 0, does not decrease and ends at nnz";
        else if (D)
            what = "col[" + std::to_string(p - R - 1) + "] = " + std::to_string(v) + " with F = n / D = " + std::to_string(c->n) +
                   " / " + std::to_string(D) + " = " + std::to_string(n) + ": a column index lies in [0, F)";
        else
            what = "col[" + std::to_string(p - R - 1) + "] = " + std::to_string(v) + " with n = " + std::to_string(n) +
                   ": a column index lies in [0, n)";
        set_error(name + what + "; " + std::to_string(got[0]) + " of the " + std::to_string(R + 1 + nnz) +
                  " positions of rowptr and col offend, this is the first");
        return LBFGSX_E_INVALID;
    }
    l.R = R;
    l.nnz = nnz;
    l.C = kLinearChunk;
    l.D = D;
    l.L = lanes ? lanes : linear_lanes_rule(R, nnz);
    // the transposed list
    uint32_t *kin = nullptr, *kout = nullptr, *vin = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kin), size_t(nnz) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&kout), size_t(nnz) * 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&vin), size_t(nnz) * 4));
    LBFGSX_HIP(own(&l.tpos, size_t(nnz) * 4));
    LBFGSX_HIP(own(&l.colptr, size_t(n + 1) * 4));
    LBFGSX_HIP(own(&l.trow, size_t(nnz) * 4));
    LBFGSX_HIP(own(&l.tval, size_t(nnz) * esz));
    LBFGSX_HIP(own(&l.w, size_t(R) * Dw * esz));
    LBFGSX_HIP(own(&l.v, size_t(R) * esz));
    uint32_t* tpos = static_cast<uint32_t*>(l.tpos);
    uint32_t* colptr = static_cast<uint32_t*>(l.colptr);
    LBFGSX_LAUNCH(k_lin_expand, dim3(grid_of(nnz)), dim3(kBlock), 0, c->stream, dcol, nnz, kin, vin);
    unsigned end_bit = 1;
    while (end_bit < 32 && (uint64_t(n - 1) >> end_bit) != 0)
        end_bit++;
    size_t bytes = 0;
    void* tmp = nullptr;
    LBFGSX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, tpos, size_t(nnz), 0, end_bit, c->stream));
    LBFGSX_HIP(t.get(&tmp, bytes));
    counters().launches.fetch_add(1, std::memory_order_relaxed);
    LBFGSX_HIP(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, tpos, size_t(nnz), 0, end_bit, c->stream));
    LBFGSX_LAUNCH(k_lin_colptr, dim3(grid_of(n + 1)), dim3(kBlock), 0, c->stream, kout, nnz, n, colptr);
    if (c->dtype == LBFGSX_F64)
        LBFGSX_LAUNCH((k_lin_entries<double>), dim3(grid_of(nnz)), dim3(kBlock), 0, c->stream, drow,
                      static_cast<const double*>(l.val), tpos, R, nnz, static_cast<int32_t*>(l.trow), static_cast<double*>(l.tval));
    else
        LBFGSX_LAUNCH((k_lin_entries<float>), dim3(grid_of(nnz)), dim3(kBlock), 0, c->stream, drow,
                      static_cast<const float*>(l.val), tpos, R, nnz, static_cast<int32_t*>(l.trow), static_cast<float*>(l.tval));
    // the long columns
    const unsigned int cap = unsigned(nnz / (int64_t(l.C) + 1) + 1);
    unsigned int* cnt = nullptr;
    uint32_t* list = nullptr;
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&cnt), 4));
    LBFGSX_HIP(t.get(reinterpret_cast<void**>(&list), size_t(cap) * 12));
    LBFGSX_HIP(hipMemsetAsync(cnt, 0, 4, c->stream));
    LBFGSX_LAUNCH(k_lin_find_long, dim3(grid_of(n)), dim3(kBlock), 0, c->stream, colptr, n, uint32_t(l.C), cap, cnt, list);
    unsigned int nlong = 0;
    LBFGSX_HIP(copy_async(&nlong, cnt, 4, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(stream_sync(c->stream));
    if (nlong > cap)
    {
        set_error(name + "more long columns than nnz / (C + 1) allows: the list is inconsistent");
        return LBFGSX_E_LOGIC;
    }
    l.nlong = int(nlong);
    l.nchunks = 0;
    if (nlong)
    {
        std::vector<uint32_t> h(size_t(nlong) * 3);
        LBFGSX_HIP(copy_async(h.data(), list, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(stream_sync(c->stream));
        std::vector<size_t> order(nlong);
        for (size_t k = 0; k < order.size(); k++)
            order[k] = k;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h[3 * a] < h[3 * b]; });
        std::vector<int32_t> lcol(nlong);
        std::vector<uint32_t> lchunk(size_t(nlong) + 1), chunk;
        for (size_t k = 0; k < order.size(); k++)
        {
            const uint32_t j = h[3 * order[k]], lo = h[3 * order[k] + 1], hi = h[3 * order[k] + 2];
            lcol[k] = int32_t(j);
            lchunk[k] = uint32_t(chunk.size() / 2);
            for (uint64_t b = lo; b < hi; b += uint64_t(l.C))
            {
                chunk.push_back(uint32_t(b));
                chunk.push_back(uint32_t(std::min<uint64_t>(b + uint64_t(l.C), hi)));
            }
        }
        lchunk[nlong] = uint32_t(chunk.size() / 2);
        l.nchunks = int64_t(chunk.size() / 2);
        LBFGSX_HIP(own(&l.long_col, lcol.size() * 4));
        LBFGSX_HIP(own(&l.long_chunk, lchunk.size() * 4));
        LBFGSX_HIP(own(&l.chunk, chunk.size() * 4));
        LBFGSX_HIP(own(&l.part, size_t(l.nchunks) * Dw * esz));
        LBFGSX_HIP(copy_async(l.long_col, lcol.data(), lcol.size() * 4, hipMemcpyHostToDevice, c->stream));
        LBFGSX_HIP(copy_async(l.long_chunk, lchunk.data(), lchunk.size() * 4, hipMemcpyHostToDevice, c->stream));
        LBFGSX_HIP(copy_async(l.chunk, chunk.data(), chunk.size() * 4, hipMemcpyHostToDevice, c->stream));
        LBFGSX_HIP(stream_sync(c->stream));  // the host vectors go when this returns
    }
    return LBFGSX_OK;
}

}  // namespace

// The lanes that share a row in the row pass: the largest power of two <= max(1, nnz / R), capped at 64 (one wavefront).  A
// row of the average length then gives every lane one entry or two, and the log2(L) cross-lane steps stay a small share of
// the row's work; rows much longer than the average loop, rows much shorter leave lanes idle.
int linear_lanes_rule(int64_t R, int64_t nnz)
{
    const int64_t avg = R > 0 ? nnz / R : 1;
    int L = 1;
    while (L < 64 && int64_t(L) * 2 <= avg)
        L *= 2;
    return L;
}

void linear_topology_free(lbfgsx_ctx* c)
{
    lbfgsx_ctx::LinearTopo& l = c->lin;
    void* all[] = {l.rowptr, l.col, l.val, l.colptr, l.trow, l.tval, l.tpos, l.w, l.v, l.part, l.long_col, l.long_chunk, l.chunk};
    for (void* p : all)
        (void) hipFree(p);
    l = lbfgsx_ctx::LinearTopo();
}

int linear_topology_build(lbfgsx_ctx* c, int64_t R, int64_t nnz, const int32_t* rowptr, const int32_t* col, const void* val,
                          int on_device, int lanes, int D, bool beside_graph)
{
    LBFGSX_HIP(stream_sync(c->stream));  // no launch of an earlier binding still walks the list this call frees
    if (!beside_graph)
        graph_topology_free(c);
    const int rc = build(c, R, nnz, rowptr, col, val, on_device, lanes, D);
    if (rc)
    {
        (void) stream_sync(c->stream);
        linear_topology_free(c);
    }
    return rc;
}

int linear_topology_read(lbfgsx_ctx* c, uint32_t* colptr, int32_t* trow, uint32_t* tpos, int32_t* long_col, uint32_t* long_chunk,
                         uint32_t* chunk)
{
    const lbfgsx_ctx::LinearTopo& l = c->lin;
    if (colptr)
        LBFGSX_HIP(copy_async(colptr, l.colptr, size_t((l.D ? c->n / l.D : c->n) + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (trow)
        LBFGSX_HIP(copy_async(trow, l.trow, size_t(l.nnz) * 4, hipMemcpyDeviceToHost, c->stream));
    if (tpos)
        LBFGSX_HIP(copy_async(tpos, l.tpos, size_t(l.nnz) * 4, hipMemcpyDeviceToHost, c->stream));
    if (l.nlong)
    {
        if (long_col)
            LBFGSX_HIP(copy_async(long_col, l.long_col, size_t(l.nlong) * 4, hipMemcpyDeviceToHost, c->stream));
        if (long_chunk)
            LBFGSX_HIP(copy_async(long_chunk, l.long_chunk, size_t(l.nlong + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        if (chunk)
            LBFGSX_HIP(copy_async(chunk, l.chunk, size_t(l.nchunks) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    LBFGSX_HIP(stream_sync(c->stream));
    return LBFGSX_OK;
}

int linear_long_launch(lbfgsx_ctx* c)
{
    const lbfgsx_ctx::LinearTopo& l = c->lin;
    if (!l.nlong)
        return LBFGSX_OK;
    const uint32_t* chunk = static_cast<const uint32_t*>(l.chunk);
    const int32_t* trow = static_cast<const int32_t*>(l.trow);
    const int D = l.D ? l.D : 1;  // the scalar form binds with D = 0
    const unsigned blocks = unsigned(l.nchunks) * unsigned(D);
    if (c->dtype == LBFGSX_F64)
        LBFGSX_LAUNCH((k_lin_long_cols<double>), dim3(blocks), dim3(kBlock), 0, c->stream, chunk, trow,
                      static_cast<const double*>(l.tval), static_cast<const double*>(l.w), static_cast<double*>(l.part), D);
    else
        LBFGSX_LAUNCH((k_lin_long_cols<float>), dim3(blocks), dim3(kBlock), 0, c->stream, chunk, trow,
                      static_cast<const float*>(l.tval), static_cast<const float*>(l.w), static_cast<float*>(l.part), D);
    return LBFGSX_OK;
}

}  // namespace lbfgsx
