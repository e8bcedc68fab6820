// lbfgspp_amd/csrc/lbfgsb_cauchy.hip -- L-BFGS-B device operators of the generalised Cauchy point: the build of the break points, their full
// and partial sorts, the chunks of the host search, the device search (gcp_scan.cuh), the finish and the subspace's opening.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gcp_scan.cuh"

#define LBFGSB_TU "lbfgsb_cauchy"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

template <class T>
struct KeyLE
{
    T tau;
    __device__ bool operator()(const T& k) const { return k <= tau; }
};
template <class T>
__global__ void k_gather_keys(const T* __restrict__ keys, const int* __restrict__ idx, T* __restrict__ out, int64_t count)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < count; k += stride)
        out[k] = keys[idx[k]];
}
// The partial sort of a SHORT candidate list in one block (round 5).  In steady state the build lists 10^1..10^3 rows whose
// break point is below the threshold; ordering them took three launches -- a radix sort of the row numbers, the gather of their
// keys, a stable radix sort by key: 30 us of launches and passes for a few KB, every iteration, ahead of the W'd pass.  Here one
// block sorts the (key, row) pairs in LDS by the order those two sorts produce together -- by key in the radix sort's own order
// (the sign-magnitude bits made monotone; -0.0 and +0.0 equal, as rocprim's codec has it), rows ascending among equal keys;
// rows are distinct, so the order is total and the bitonic network's lack of stability does not matter.  9-19 us less per
// iteration (scripts/r5/chain_ab.sh, profiles/r5_chain_ab.txt).
// (The same block also gathering the first chunk of the host search -- [brk | g | z | W rows] of the first 512 sorted break
// points, instead of the column table's upload + k_cauchy_gather -- was measured in two forms, into the copy's source buffer
// and straight into host-mapped memory: 4-7 us SLOWER than the separate launches either way, one CU's worth of outstanding
// loads against two and an upload that overlaps the sort.  Not kept.)
// Steps whose partners are less than 64 apart stay inside the 128 elements one wavefront handles: no block barrier there.
constexpr int kPselSmallCap = 4096;
constexpr int kPselSmallThreads = 1024;
template <class T>
struct KeyBits;
template <>
struct KeyBits<double>
{
    typedef unsigned long long U;
    static constexpr U sign = 0x8000000000000000ull;
};
template <>
struct KeyBits<float>
{
    typedef unsigned U;
    static constexpr U sign = 0x80000000u;
};
template <class T>
__global__ void __launch_bounds__(kPselSmallThreads)
    k_psel_sort_small(const int* __restrict__ list, int cnt, const T* __restrict__ keys, T* __restrict__ keys_out,
                      int* __restrict__ vals_out)
{
    typedef typename KeyBits<T>::U U;
    constexpr U sign = KeyBits<T>::sign;
    __shared__ U sk[kPselSmallCap];
    __shared__ int si[kPselSmallCap];
    int P = 128;  // at least one wavefront's span
    while (P < cnt)
        P <<= 1;
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += kPselSmallThreads)
    {
        U e = ~U(0);
        int r = 0x7FFFFFFF;
        if (i < cnt)
        {
            r = list[i];
            const U bits = __builtin_bit_cast(U, keys[r]);
            e = bits ^ ((bits & sign) ? ~U(0) : sign);
        }
        sk[i] = e;
        si[i] = r;
    }
    // (the padding sorts behind every real pair: its row is larger than any row, its key not smaller than any key)
    auto canon = [](U e) { return e == U(~sign) ? sign : e; };  // -0.0 as +0.0
    int prev_j = 64;  // the loads above were by other wavefronts
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
        {
            // pair t of a step touches elements 2 (t - t % j) + t % j and that + j: for j < 64 the 64 pairs of a wavefront's
            // pass stay inside one aligned run of 128 elements, the same run for every such j -- a wavefront's LDS
            // operations execute in order, so only the compiler has to be kept from moving them
            if (j >= 64 || prev_j >= 64)
                __syncthreads();
            else
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            prev_j = j;
            for (int t = tid; t < (P >> 1); t += kPselSmallThreads)
            {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
                const U a = sk[i], b = sk[x];
                const int ra = si[i], rb = si[x];
                const U ca = canon(a), cb = canon(b);
                const bool gt = ca > cb || (ca == cb && ra > rb);
                const bool asc = (i & k) == 0;
                if (gt == asc)
                {
                    sk[i] = b;
                    sk[x] = a;
                    si[i] = rb;
                    si[x] = ra;
                }
            }
        }
    __syncthreads();
    auto key_at = [&](int i) {
        const U e = sk[i];
        return __builtin_bit_cast(T, U(e ^ ((e & sign) ? sign : ~U(0))));
    };
    for (int i = tid; i < cnt; i += kPselSmallThreads)
    {
        keys_out[i] = key_at(i);
        vals_out[i] = si[i];
    }
}
static std::atomic<int64_t> g_psel_small{0};
size_t sort_pairs_tmp_bytes(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    size_t bytes = 0;
    if (c->dtype == LBFGSX_F64)
        (void) rocprim::radix_sort_pairs(nullptr, bytes, P<double>(b->keys_in), P<double>(b->keys_out), b->vals_in,
                                         b->vals_out, size_t(c->n), 0, 64, c->stream);
    else
        (void) rocprim::radix_sort_pairs(nullptr, bytes, P<float>(b->keys_in), P<float>(b->keys_out), b->vals_in,
                                         b->vals_out, size_t(c->n), 0, 32, c->stream);
    return bytes;
}
// buffers of the compact copy and the positions of the 64-row batches for the current free set; false: do without
bool wf_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    const int64_t nbatch = (c->n + 63) / 64;
    if (!b->wf)
    {
        const size_t esz = (c->dtype == LBFGSX_F64) ? 8 : 4;
        b->wf_ld = c->ld;
        size_t bytes = 0;
        bool ok = hipMalloc(&b->wf, esz * size_t(b->wf_ld) * size_t(std::max(32, 2 * c->m))) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&b->wf_idx), sizeof(int) * size_t(c->n)) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&b->wf_pos), sizeof(int) * size_t(c->n)) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&b->wf_cnt), sizeof(int) * size_t(nbatch + 2)) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&b->wf_base), sizeof(int) * size_t(nbatch + 2)) == hipSuccess &&
                  rocprim::exclusive_scan(nullptr, bytes, b->wf_cnt, b->wf_base, 0, size_t(nbatch + 1), rocprim::plus<int>(),
                                          c->stream) == hipSuccess &&
                  hipMalloc(&b->wf_tmp, std::max<size_t>(bytes, 16)) == hipSuccess;
        b->wf_tmp_bytes = bytes;
        if (!ok)
        {
            (void) hipGetLastError();
            (void) hipFree(b->wf);
            (void) hipFree(b->wf_idx);
            (void) hipFree(b->wf_cnt);
            (void) hipFree(b->wf_base);
            (void) hipFree(b->wf_tmp);
            (void) hipFree(b->wf_pos);
            b->wf = b->wf_tmp = nullptr;
            b->wf_idx = b->wf_cnt = b->wf_base = b->wf_pos = nullptr;
            b->wf_use = false;  // no room for the copy: the masked passes do the work
            return false;
        }
    }
    return true;
}
bool wf_prepare(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    const int64_t nbatch = (c->n + 63) / 64;
    if (!wf_alloc(c))
        return false;
    b->wf_live = false;
    if (hipMemsetAsync(b->wf_pos, 0xFF, sizeof(int) * size_t(c->n), c->stream) != hipSuccess)  // every position -1
    {
        (void) hipGetLastError();
        return false;
    }
    const int grid = int(std::min<int64_t>(c->grid_for(c->n), (nbatch + 4) / 4));
    LBFGSX_LAUNCH(k_free_counts, dim3(std::max(1, grid)), dim3(kBlock), 0, c->stream, c->bstate->st, c->n, nbatch, b->wf_cnt);
    size_t bytes = b->wf_tmp_bytes;
    if (rocprim::exclusive_scan(b->wf_tmp, bytes, b->wf_cnt, b->wf_base, 0, size_t(nbatch + 1), rocprim::plus<int>(), c->stream) !=
        hipSuccess)
    {
        (void) hipGetLastError();
        return false;
    }
    return true;
}
// the partial sort in two halves: the selection (launched; its count lands in `count_dev`), and the sort of the selected
// break points once the count is on the host
template <class T>
static int partial_select_t(lbfgsx_ctx* c, double tau, unsigned* count_dev)
{
    lbfgsb_state* b = c->bstate;
    {
        const int rk = ensure_keys(c);
        if (rk)
            return rk;
    }
    const size_t n = size_t(c->n);
    int rca = psort_alloc(c);
    if (rca)
        return rca;
    if (!count_dev)
        count_dev = b->pcount;
    // ordered (deterministic) compaction of the indices whose break point is <= tau ...
    rocprim::counting_iterator<int> ids(0);
    rocprim::transform_iterator<const T*, KeyLE<T>, bool> flags(P<T>(b->keys_in), KeyLE<T>{T(tau)});
    size_t bytes = 0;
    LBFGSX_HIP(rocprim::select(nullptr, bytes, ids, flags, b->pv, count_dev, n, c->stream));
    if (bytes > b->sel_tmp_bytes)
    {
        (void) hipFree(b->sel_tmp);
        LBFGSX_HIP(hipMalloc(&b->sel_tmp, bytes));
        b->sel_tmp_bytes = bytes;
    }
    LBFGSX_HIP(rocprim::select(b->sel_tmp, bytes, ids, flags, b->pv, count_dev, n, c->stream));
    return LBFGSX_OK;
}
// buffers of the in-pass selection (k_cauchy_build's plist); false: do without
bool psel_alloc(lbfgsx_ctx* c)
{
    lbfgsb_state* b = c->bstate;
    if (b->psel_list)
        return true;
    b->psel_cap = unsigned(std::min<int64_t>(b->psel_cap, c->n));
    size_t bytes = 0;
    const bool ok = psort_alloc(c) == LBFGSX_OK &&
                    hipMalloc(reinterpret_cast<void**>(&b->psel_list), sizeof(int) * size_t(b->psel_cap)) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void**>(&b->psel_cnt), sizeof(unsigned)) == hipSuccess &&
                    hipMemsetAsync(b->psel_cnt, 0, sizeof(unsigned), c->stream) == hipSuccess &&
                    rocprim::radix_sort_keys(nullptr, bytes, b->psel_list, b->pv, size_t(b->psel_cap), 0, 32, c->stream) == hipSuccess &&
                    hipMalloc(&b->psel_tmp, std::max<size_t>(bytes, 16)) == hipSuccess;
    if (!ok)
    {
        (void) hipGetLastError();
        (void) hipFree(b->psel_list);
        (void) hipFree(b->psel_cnt);
        (void) hipFree(b->psel_tmp);
        b->psel_list = nullptr;
        b->psel_cnt = nullptr;
        b->psel_tmp = nullptr;
        b->psel_use = false;
        return false;
    }
    b->psel_tmp_bytes = bytes;
    return true;
}
template <class T>
static int partial_sort_tail_t(lbfgsx_ctx* c, unsigned cnt, int64_t* nsorted)
{
    lbfgsb_state* b = c->bstate;
    *nsorted = int64_t(cnt);
    if (cnt == 0)
        return LBFGSX_OK;
    // ... their keys, and a stable sort of that short list: the same order the full sort gives these entries
    const int grid = int(std::min<int64_t>((int64_t(cnt) + 255) / 256, 1024));
    // (the listed candidates are ordered break points: their key IS their break point, whether or not the build wrote keys_in)
    LBFGSX_LAUNCH((k_gather_keys<T>), dim3(grid), dim3(256), 0, c->stream, b->keys_valid ? P<T>(b->keys_in) : static_cast<T*>(b->brk),
                  b->pv, P<T>(b->pk), int64_t(cnt));
    size_t sbytes = b->sort_tmp_bytes;
    lbfgsx::model_add(double(cnt) * (96.0 + 64.0 + 2 * sizeof(T)));  // byte model: the candidates' keys gathered (a sector each) and sorted
    LBFGSX_HIP(rocprim::radix_sort_pairs(b->sort_tmp, sbytes, P<T>(b->pk), P<T>(b->keys_out), b->pv, b->vals_out, size_t(cnt), 0,
                                         int(sizeof(T) * 8), c->stream));
    return LBFGSX_OK;
}
// the partial sort over the candidates the build listed: rows in ascending order first -- what an ordered compaction
// delivers, and what makes the stable sort by break point put ties in the reference's order -- then as partial_sort_tail_t
template <class T>
static int partial_sort_listed_t(lbfgsx_ctx* c, unsigned cnt, int64_t* nsorted)
{
    lbfgsb_state* b = c->bstate;
    if (b->psel_small && cnt >= 1 && cnt <= unsigned(kPselSmallCap))
    {
        // (the listed candidates are ordered break points: their key IS their break point, whether or not the build wrote keys_in)
        *nsorted = int64_t(cnt);
        g_psel_small++;
        lbfgsx::model_add(double(cnt) * (64.0 + 4 + 2 * (sizeof(T) + 4)));  // byte model: the list, a sector per key, the sorted pairs out
        LBFGSX_LAUNCH((k_psel_sort_small<T>), dim3(1), dim3(kPselSmallThreads), 0, c->stream, b->psel_list, int(cnt),
                      b->keys_valid ? P<T>(b->keys_in) : static_cast<T*>(b->brk), P<T>(b->keys_out), b->vals_out);
        LBFGSX_HIP(hipGetLastError());
        return LBFGSX_OK;
    }
    if (cnt > 1)
    {
        size_t bytes = b->psel_tmp_bytes;
        int end_bit = 1;
        while (end_bit < 32 && (int64_t(1) << end_bit) < c->n)
            end_bit++;
        LBFGSX_HIP(rocprim::radix_sort_keys(b->psel_tmp, bytes, b->psel_list, b->pv, size_t(cnt), 0, end_bit, c->stream));
    }
    else if (cnt == 1)
        LBFGSX_HIP(lbfgsx::copy_async(b->pv, b->psel_list, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    return partial_sort_tail_t<T>(c, cnt, nsorted);
}
template <class T>
static int partial_sort_t(lbfgsx_ctx* c, double tau, int64_t* nsorted)
{
    lbfgsb_state* b = c->bstate;
    int rc = partial_select_t<T>(c, tau, nullptr);
    if (rc)
        return rc;
    unsigned cnt = 0;
    LBFGSX_HIP(lbfgsx::copy_async(&cnt, b->pcount, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return partial_sort_tail_t<T>(c, cnt, nsorted);
}
// gather kernel + ONE copy of [brk | g | z | W rows] of sorted positions [first, first + count) into the landing zone `*land`
// (pinned when it fits, else `pageable`); nothing is waited for
static int cauchy_chunk_launch(lbfgsx_ctx* c, int64_t first, int64_t count, bool with_w, int* idx, double** land,
                               std::vector<double>* pageable)
{
    lbfgsb_state* b = c->bstate;
    const int nc = c->ncorr;
    // one packed device buffer [brk | g | z | W rows] of (3 + 2c) * count doubles and ONE copy back (four separate copies
    // were four blit kernels per chunk); the pinned landing zone serves the chunks the host form actually asks for
    const size_t per = size_t(3 + 2 * nc);
    // sized for the full history: 2c grows over the first m iterations, and a free + two allocations in the middle of each
    // of them cost 0.3-0.4 ms apiece
    const size_t per_cap = size_t(3 + 2 * c->m);
    if (count > b->g_cap || c->m != b->g_ncorr)
    {
        void* old[] = {b->g_brk, b->g_idx};
        for (void* p : old)
            (void) hipFree(p);
        b->g_brk = nullptr;
        b->g_idx = nullptr;
        const int64_t cap = std::max<int64_t>(count, b->g_cap);
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->g_brk), sizeof(double) * size_t(cap) * per_cap));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->g_idx), sizeof(int) * size_t(cap)));
        b->g_cap = cap;
        b->g_ncorr = c->m;
    }
    double* d_brk = b->g_brk;
    double* d_g = d_brk + count;
    double* d_z = d_g + count;
    double* d_w = d_z + count;
    int rc = upload_phys(c);
    if (rc)
        return rc;
    const int grid = int(std::min<int64_t>((count + 255) / 256, 2048));
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        LBFGSX_LAUNCH((k_cauchy_gather<T>), dim3(grid), dim3(256), 0, c->stream, bv, P<T>(b->keys_out), b->vals_out, first,
                           count, P<T>(c->S), P<T>(c->Y), c->ld, b->phys_dev, nc, d_brk, d_g, d_z, b->g_idx, d_w);
    });
    LBFGSX_HIP(hipGetLastError());
    const size_t ndbl = size_t(count) * ((nc > 0 && with_w) ? per : size_t(3));
    if (ndbl > b->g_host_cap)
    {
        if (b->g_host)
            (void) hipHostFree(b->g_host);
        b->g_host = nullptr;
        b->g_host_cap = 0;
        const size_t want = std::max<size_t>(ndbl, size_t(1) << 16);
        if (want <= (size_t(1) << 25))  // up to 256 MB pinned; larger chunks land in a pageable buffer
        {
            LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->g_host), sizeof(double) * want, hipHostMallocDefault));
            b->g_host_cap = want;
        }
    }
    *land = b->g_host;
    if (ndbl > b->g_host_cap)
    {
        if (!pageable)
            return LBFGSX_E_INVALID;
        pageable->resize(ndbl);
        *land = pageable->data();
    }
    LBFGSX_HIP(lbfgsx::copy_async(*land, d_brk, sizeof(double) * ndbl, hipMemcpyDeviceToHost, c->stream));
    if (idx)
        LBFGSX_HIP(lbfgsx::copy_async(idx, b->g_idx, sizeof(int) * size_t(count), hipMemcpyDeviceToHost, c->stream));
    return LBFGSX_OK;
}
// ---- device GCP search over sorted positions [first, first + count) (gcp_scan.cuh) ----------------------------
template <int NC>
static int gcp_scan_nc(lbfgsx_ctx* c, const GcpBufs& gb, int64_t first, int64_t count, int64_t nord, double theta,
                       double t_prev)
{
    lbfgsb_state* b = c->bstate;
    const int nc = c->ncorr;
    const int ntiles = int((count + kGcpTile - 1) / kGcpTile);
    // s_small: [0, NC*NC) M | init A (NC) | init B (NC+1) | init C (1) | fin (NC+1) | out (2NC+4)
    double* M = b->s_small;
    double* initA = M + NC * NC;
    double* initB = initA + NC;
    double* initC = initB + NC + 1;
    double* fin = initC + 1;
    double* out = fin + NC + 1;
    hipStream_t st = c->stream;
    LBFGSX_LAUNCH((k_gcp_a1<NC>), dim3(ntiles), dim3(kGcpTile), 0, st, gb, count, nc, theta, b->s_ts);
    LBFGSX_LAUNCH(k_gcp_tiles, dim3(NC), dim3(64), 0, st, b->s_ts, b->s_off, ntiles, NC, initA, fin);
    LBFGSX_LAUNCH((k_gcp_a3b1<NC>), dim3(ntiles), dim3(kGcpTile), 0, st, gb, count, nc, theta, t_prev, M, b->s_off, b->s_ts);
    LBFGSX_LAUNCH(k_gcp_tiles, dim3(NC + 1), dim3(64), 0, st, b->s_ts, b->s_off, ntiles, NC + 1, initB, fin);
    if (b->chain_host)
    {
        // exact-order mode: per-crossing terms only; the chains and the exit test run on the host (gcp_chain_host)
        LBFGSX_LAUNCH((k_gcp_b3c1<NC, true>), dim3(ntiles), dim3(kGcpTile), 0, st, gb, count, nc, theta, t_prev, M,
                           b->s_off, b->s_ts, first, nord);
        LBFGSX_HIP(hipGetLastError());
        return LBFGSX_OK;
    }
    LBFGSX_LAUNCH((k_gcp_b3c1<NC, false>), dim3(ntiles), dim3(kGcpTile), 0, st, gb, count, nc, theta, t_prev, M, b->s_off, b->s_ts, first, nord);
    LBFGSX_LAUNCH(k_gcp_tiles, dim3(1), dim3(64), 0, st, b->s_ts, b->s_off, ntiles, 1, initC, fin);
    LBFGSX_LAUNCH(k_gcp_c3, dim3(ntiles), dim3(kGcpTile), 0, st, gb, count, first, nord, b->s_off, b->s_exit);
    LBFGSX_LAUNCH((k_gcp_extract<NC>), dim3(1), dim3(64), 0, st, gb, count, nc, theta, b->s_exit, out);
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}
template <int NC>
static void gcp_extract_nc(lbfgsx_ctx* c, const GcpBufs& gb, int64_t count, double theta)
{
    lbfgsb_state* b = c->bstate;
    LBFGSX_LAUNCH((k_gcp_extract<NC>), dim3(1), dim3(64), 0, c->stream, gb, count, c->ncorr, theta, b->exit_map_dev, b->gout_dev);
}

// The f' / f'' recurrences of the break-point search in the reference's own order (Cauchy.h:218,227-228,240-256) over
// the per-crossing terms a chunk of the device search produced: dt[k] (0 inside a group of ties, where the statements
// the reference executes once per group are exact no-ops), A[k] (added to f'), B[k] (subtracted from f'').
// dt[count] = distance to the break point after the chunk, -1 at the end of the sorted list.  Returns the index of the
// group end at which the search stops, or -1.  Plain IEEE operations, no contraction (the TU is built with
// -ffp-contract=off): bit for bit the scalar statements of the sequential form.
// CT: the scalar type of the problem.  An f32 reference runs these chains in float, and over 10^5 crossings the float
// rounding of f' (partial sums of the size of d'd) moves the Cauchy point far more than the f32 tolerance: the chain is
// part of what has to be reproduced, so f32 problems run it in float over the (double-computed, then rounded) terms.
template <class CT>
static int64_t gcp_chain_host(const double* dt, const double* A, const double* B, int64_t k0, int64_t k1, double& fp, double& fpp)
{
    // crossings [k0, k1) of the chunk; f' and f'' go in and out through fp, fpp (exact for CT = float too: a float
    // widened to double and back is the same float), so a chunk can be walked in pieces as its terms arrive
    CT f1 = CT(fp), f2 = CT(fpp);
    for (int64_t k = k0; k < k1; k++)
    {
        f1 = f1 + CT(dt[k]) * f2;   // fp += deltat * fpp                                   (:218)
        f1 = f1 + CT(A[k]);         // fp += ggact + theta*gact*zact - gact*cache.dot(vecc)  (:227)
        f2 = f2 - CT(B[k]);         // fpp -= (...)                                          (:228)
        const CT dn = CT(dt[k + 1]);
        if (dn > CT(0) && !(-f1 / f2 >= dn))   // group end: deltatmin = -fp/fpp (:240) against the next deltat (:183)
        {
            fp = double(f1);
            fpp = double(f2);
            return k;
        }
    }
    fp = double(f1);
    fpp = double(f2);
    return -1;
}
// buffers of the device break-point search for chunks of up to `count` crossings and NC components
int scan_alloc(lbfgsx_ctx* c, int64_t count, int NC)
{
    lbfgsb_state* b = c->bstate;
    if (count > b->s_cap || NC > b->s_nc)
    {
        void* old[] = {b->s_brk, b->s_g, b->s_z, b->s_W, b->s_P, b->s_C, b->s_chain, b->s_ts, b->s_off};
        for (void* p : old)
            (void) hipFree(p);
        // sized once for the largest chunk the search asks for (2^20 crossings, or all n coordinates) and the full
        // history: the chunk grows 2^16 -> 2^20 within a search and 2c grows over the first m iterations, and every
        // regrowth would free and allocate eleven buffers in the middle of the iteration
        const int64_t cap = std::max<int64_t>(std::max<int64_t>(count, b->s_cap), std::min<int64_t>(int64_t(1) << 20, c->n));
        const int mcap = 2 * c->m <= 32 ? (2 * c->m + 3) / 4 * 4 : 2 * c->m <= 40 ? 40 : 2 * c->m <= 48 ? 48 : 2 * c->m <= 64 ? 64 : 80;
        const int ncap = std::max(std::max(NC, b->s_nc), mcap);
        const size_t tiles = size_t((cap + kGcpTile - 1) / kGcpTile);
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_brk), sizeof(double) * size_t(cap + 1)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_g), sizeof(double) * size_t(cap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_z), sizeof(double) * size_t(cap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_W), sizeof(double) * size_t(cap) * size_t(ncap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_P), sizeof(double) * size_t(cap) * size_t(ncap)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_C), sizeof(double) * size_t(cap) * size_t(ncap)));
        // the three per-crossing arrays the host-order chain reads share one allocation: every call lays them out back to
        // back for its own count (lbfgsx_b_cauchy_scan), so that a chunk that travels whole is one copy instead of three
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_chain), sizeof(double) * 3 * size_t(cap + 1)));
        b->s_fp = b->s_chain;
        b->s_dfp = b->s_chain + (cap + 1);
        b->s_fpp = b->s_chain + 2 * (cap + 1);
        if (b->h_chain)
            (void) hipHostFree(b->h_chain);
        b->h_chain = nullptr;
        LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->h_chain), sizeof(double) * 3 * size_t(cap + 1), hipHostMallocDefault));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_ts), sizeof(double) * tiles * size_t(ncap + 1)));
        LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_off), sizeof(double) * tiles * size_t(ncap + 1)));
        if (!b->s_small)
        {
            LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_small), sizeof(double) * (80 * 80 + 6 * 88)));
            LBFGSX_HIP(hipMalloc(reinterpret_cast<void**>(&b->s_exit), sizeof(unsigned long long)));
            LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->exit_map_host), 64, hipHostMallocMapped | hipHostMallocCoherent));
            LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->exit_map_dev), b->exit_map_host, 0));
            LBFGSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->gout_host), sizeof(double) * (2 * 80 + 8), hipHostMallocMapped | hipHostMallocCoherent));
            LBFGSX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->gout_dev), b->gout_host, 0));
        }
        b->s_cap = cap;
        b->s_nc = ncap;
    }
    return LBFGSX_OK;
}

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_cauchy_build(lbfgsx_ctx* c, int64_t* nfree, int64_t* nord, double* dd, double* wtd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const bool force = b->force_pending;  // a deferred x = clamp(x): evaluated by the build's own pass
    b->force_pending = false;
    const int grid = c->grid_for(c->n);
    double r[4] = {0, 0, 0, -1};
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        const bool wc = wtdc_prepare(c);
        const int newest = (c->ptr + c->m - 1) % c->m;
        lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(c->n) * (7 * sizeof(T) + 4));  // byte model: x, g, lb, ub read; brk, d, xcp and the index written
        b->keys_valid = b->vals_iota = true;
        LBFGSX_LAUNCH((k_cauchy_build<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, P<T>(b->keys_in), b->vals_in, c->n,
                           c->ws, b->dout, force ? P<T>(c->xb[c->cur]) : static_cast<T*>(nullptr),
                           wc ? static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)])) : static_cast<const T*>(nullptr),
                           wc ? b->wf_pos : static_cast<const int*>(nullptr), b->wtdc_list, b->wtdc_cnt, b->wtdc_cap, T(0),
                           static_cast<int*>(nullptr), static_cast<unsigned*>(nullptr), 0u);
        LBFGSX_HIP(hipGetLastError());
        rc = fetch_doubles(c, wc ? 4 : 3, r);
        if (rc)
            return rc;
        b->wtdc_n = wc ? int64_t(r[3]) : -1;
        if (r[2] > 0)
        {
            size_t bytes = b->sort_tmp_bytes;
            lbfgsx::model_add(96.0 * double(c->n));  // byte model: SURVEY 8(d)'s radix-sort figure per (key, index) pair
            LBFGSX_HIP(rocprim::radix_sort_pairs(b->sort_tmp, bytes, P<T>(b->keys_in), P<T>(b->keys_out), b->vals_in,
                                                 b->vals_out, size_t(c->n), 0, int(sizeof(T) * 8), c->stream));
        }
        // p = W'd raw dots (Cauchy.h:152)
        if (wtd && c->ncorr > 0)
        {
            rc = cauchy_wtd(c, wtd);
            if (rc)
                return rc;
        }
    });
    if (dd) *dd = r[0];
    if (nfree) *nfree = int64_t(r[1]);
    if (nord) *nord = int64_t(r[2]);
    return LBFGSX_OK;
}

int lbfgsx_b_psel_counts(int64_t out[1], int reset)
{
    if (out)
        out[0] = g_psel_small.load();
    if (reset)
        g_psel_small = 0;
    return LBFGSX_OK;
}

int lbfgsx_b_cauchy_build_partial(lbfgsx_ctx* c, double tau, int64_t* nfree, int64_t* nord, int64_t* nsorted, double* dd,
                                  double* wtd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const bool force = b->force_pending;  // a deferred x = clamp(x): evaluated by the build's own pass
    b->force_pending = false;
    const int grid = c->grid_for(c->n);
    double r[5] = {0, 0, 0, -1, -1};
    int64_t ns = 0;
    const bool tau_ok = tau > 0.0 && std::isfinite(tau);
    // the candidates of the partial sort: collected by the build itself, else selected by a pass that rides behind it
    const bool sel_inline = tau_ok && b->psel_use && b->psel_last >= 0 && b->psel_last <= lbfgsb_state::kPselMax &&
                            c->n < (int64_t(1) << 31) && psel_alloc(c);
    const bool sel_ahead = !sel_inline && b->stash_use && b->dout_host && tau_ok;
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        const bool wc = wtdc_prepare(c);
        const int newest = (c->ptr + c->m - 1) % c->m;
        // the pass of the post statements has done this one's work (lbfgsx_b_post_linesearch_build) -- if the solver is where
        // that pass assumed it would be: same iterate, same threshold and lists, and nothing for the clamp to move
        const bool from_post = b->pb_valid && b->pb_cur == c->cur && b->pb_writes == c->vec_writes && b->pb_tau == tau && b->pb_sel_inline == sel_inline &&
                               b->pb_wc == wc && !sel_ahead && (!force || b->pb_r[5] == 0.0);
        b->pb_valid = false;
        if (from_post)
        {
            for (int i = 0; i < 5; i++)
                r[i] = b->pb_r[i];
            count_pb_hit();
        }
        else
        {
        if (!sel_ahead)  // nothing rides behind the build: its last block carries the completion word
            lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(c->n) * (7 * sizeof(T) + 4));  // byte model: x, g, lb, ub read; brk, d, xcp and the index written
        b->keys_valid = b->vals_iota = true;
        LBFGSX_LAUNCH((k_cauchy_build<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, P<T>(b->keys_in), b->vals_in, c->n,
                           c->ws, b->dout, force ? P<T>(c->xb[c->cur]) : static_cast<T*>(nullptr),
                           wc ? static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)])) : static_cast<const T*>(nullptr),
                           wc ? b->wf_pos : static_cast<const int*>(nullptr), b->wtdc_list, b->wtdc_cnt, b->wtdc_cap, T(tau),
                           sel_inline ? b->psel_list : static_cast<int*>(nullptr), b->psel_cnt, b->psel_cap);
        LBFGSX_HIP(hipGetLastError());
        // the selection of the partial sort needs nothing from the host: it rides behind the build, its count lands in the
        // mapped word dout[60] and is read after the same wait (without candidates it selects nothing)
        if (sel_ahead)
        {
            rc = partial_select_t<T>(c, tau, reinterpret_cast<unsigned*>(b->dout + 60));
            if (rc)
                return rc;
        }
        rc = fetch_doubles(c, sel_inline ? 5 : wc ? 4 : 3, r);
        if (rc)
            return rc;
        }
        b->wtdc_n = wc ? int64_t(r[3]) : -1;
        ns = int64_t(r[2]);
        if (r[2] > 0)
        {
            if (tau_ok)
            {
                if (sel_inline && r[4] >= 0 && r[4] <= double(b->psel_cap))
                    rc = partial_sort_listed_t<T>(c, unsigned(r[4]), &ns);
                else if (sel_ahead)  // the selection ran behind the build: its count came with the build's sums
                    rc = partial_sort_tail_t<T>(c, *reinterpret_cast<const volatile unsigned*>(b->dout_host + 60), &ns);
                else
                    rc = partial_sort_t<T>(c, tau, &ns);
                if (rc)
                    return rc;
            }
            else
            {
                // keys_in / vals_in may have been left out by a lazy-key build (today only when tau_ok, i.e. not on this
                // branch): a no-op when they are valid, the rebuild otherwise -- never a sort of stale keys
                {
                    const int rk = ensure_keys(c);
                    if (rk)
                        return rk;
                }
                size_t bytes = b->sort_tmp_bytes;
                lbfgsx::model_add(96.0 * double(c->n));  // byte model: SURVEY 8(d)'s radix-sort figure per (key, index) pair
                LBFGSX_HIP(rocprim::radix_sort_pairs(b->sort_tmp, bytes, P<T>(b->keys_in), P<T>(b->keys_out), b->vals_in,
                                                     b->vals_out, size_t(c->n), 0, int(sizeof(T) * 8), c->stream));
            }
        }
        if (wtd && c->ncorr > 0)  // p = W'd raw dots (Cauchy.h:152)
        {
            // the host search opens with the first 512 sorted break points (Cauchy<Scalar>::Stream): their gather and copy ride
            // here, behind the sort and ahead of the W'd pass whose wait follows
            b->gpre_valid = false;
            if (b->gpre_use && ns >= 1)
            {
                double* land = nullptr;
                const int64_t cnt = std::min<int64_t>(512, ns);
                if (cauchy_chunk_launch(c, 0, cnt, true, nullptr, &land, nullptr) == LBFGSX_OK)
                {
                    b->gpre_valid = true;
                    b->gpre_count = cnt;
                    b->gpre_nc = c->ncorr;
                }
                else
                    (void) hipGetLastError();
            }
            rc = cauchy_wtd(c, wtd);
            if (rc)
            {
                b->gpre_valid = false;
                return rc;
            }
        }
    });
    b->psel_last = tau_ok ? ns : int64_t(-1);
    if (dd) *dd = r[0];
    if (nfree) *nfree = int64_t(r[1]);
    if (nord) *nord = int64_t(r[2]);
    if (nsorted) *nsorted = ns;
    return LBFGSX_OK;
}

// full sort of the break points written by the last build (after a partial one turned out too short)
int lbfgsx_b_cauchy_sort_full(lbfgsx_ctx* c)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    b->gpre_valid = false;
    rc = ensure_keys(c);
    if (rc)
        return rc;
    DISPATCH_T(c, {
        size_t bytes = b->sort_tmp_bytes;
        lbfgsx::model_add(96.0 * double(c->n));  // byte model: SURVEY 8(d)'s radix-sort figure per (key, index) pair
        LBFGSX_HIP(rocprim::radix_sort_pairs(b->sort_tmp, bytes, P<T>(b->keys_in), P<T>(b->keys_out), b->vals_in, b->vals_out,
                                             size_t(c->n), 0, int(sizeof(T) * 8), c->stream));
    });
    return LBFGSX_OK;
}

int lbfgsx_b_cauchy_chunk(lbfgsx_ctx* c, int64_t first, int64_t count, double* brk, double* g, double* z, int* idx,
                          double* wrows)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    if (count <= 0)
        return LBFGSX_OK;
    const int nc = c->ncorr;
    double* land = nullptr;
    std::vector<double> pageable;
    const bool ahead = b->gpre_valid && first == 0 && count == b->gpre_count && nc == b->gpre_nc && !idx && (wrows || nc == 0);
    b->gpre_valid = false;
    if (ahead)
        land = b->g_host;  // launched by the build, landed with the wait of its W'd pass
    else
    {
        rc = cauchy_chunk_launch(c, first, count, wrows != nullptr, idx, &land, &pageable);
        if (rc)
            return rc;
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    }
    std::memcpy(brk, land, sizeof(double) * size_t(count));
    std::memcpy(g, land + count, sizeof(double) * size_t(count));
    std::memcpy(z, land + 2 * count, sizeof(double) * size_t(count));
    if (nc > 0 && wrows)
        std::memcpy(wrows, land + 3 * count, sizeof(double) * size_t(count) * size_t(2 * nc));
    return LBFGSX_OK;
}

int lbfgsx_b_cauchy_scan(lbfgsx_ctx* c, int64_t first, int64_t count, int64_t nord, const double* Mmat, double theta,
                         double t_prev, const double* state_in, int64_t* exit_at, double* state_out)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int nc = c->ncorr, nc2 = 2 * nc;
    if (nc2 > 80 || count < 1 || first < 0 || first + count > nord)
    {
        set_error("lbfgsx_b_cauchy_scan: needs 2*ncorr <= 80 and a non-empty range inside the sorted list");
        return LBFGSX_E_INVALID;
    }
    // component counts the kernels are built for: multiples of 4 up to 32, then 40, 48, 64, 80 (m = 20, 24, 32, 40)
    const int NC = nc2 <= 32 ? std::max(4, (nc2 + 3) / 4 * 4) : nc2 <= 40 ? 40 : nc2 <= 48 ? 48 : nc2 <= 64 ? 64 : 80;
    rc = scan_alloc(c, count, NC);
    if (rc)
        return rc;
    rc = upload_phys(c);
    if (rc)
        return rc;
    // small inputs in one staged copy: padded M (row-major NC x NC), the three scan seeds
    std::vector<double> hbuf(size_t(80 * 80 + 6 * 88), 0.0);
    double* h = hbuf.data();
    for (int i = 0; i < nc2; i++)
        for (int j = 0; j < nc2; j++)
            h[i * NC + j] = Mmat[size_t(j) * size_t(nc2) + size_t(i)];
    double* initA = h + NC * NC;
    double* initB = initA + NC;
    double* initC = initB + NC + 1;
    for (int j = 0; j < nc2; j++)
    {
        initA[j] = state_in[j];        // p
        initB[j] = state_in[nc2 + j];  // c
    }
    initB[NC] = state_in[2 * nc2 + 1];  // f''
    initC[0] = state_in[2 * nc2];       // f'
    const size_t nsmall = size_t(NC * NC + NC + NC + 1 + 1);
    LBFGSX_HIP(lbfgsx::copy_async(b->s_small, h, sizeof(double) * nsmall, hipMemcpyHostToDevice, c->stream));
    if (!b->chain_host)
        LBFGSX_HIP(hipMemsetAsync(b->s_exit, 0xFF, sizeof(unsigned long long), c->stream));
    const int grid = int(std::min<int64_t>((count + 256) / 256, 2048));
    // f32 problems: the sorted list is gathered into doubles and the search runs in double (the reference would run it in
    // float; the north_star tolerance for f32 is 1e-4, the difference is at the 1e-7 level)
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_gcp_gather<T>), dim3(grid), dim3(256), 0, c->stream, bvecs<T>(c), P<T>(b->keys_out), b->vals_out,
                           first, count, nord, P<T>(c->S), P<T>(c->Y), c->ld, b->phys_dev, nc, b->s_brk, b->s_g, b->s_z, b->s_W,
                           b->s_cap);
    });
    // the three per-crossing arrays of this call, back to back in s_chain (pitch count + 1, not the capacity): a chunk that
    // travels whole is ONE linear copy (hipMemcpy2DAsync over a capacity pitch was tried: it stalls for 20 ms now and then)
    b->s_fp = b->s_chain;
    b->s_dfp = b->s_chain + (count + 1);
    b->s_fpp = b->s_chain + 2 * (count + 1);
    GcpBufs gb = {b->s_brk, b->s_g, b->s_z, b->s_W, b->s_P, b->s_C, b->s_fpp, b->s_dfp, b->s_fp, b->s_cap};
    switch (NC)
    {
    case 4: rc = gcp_scan_nc<4>(c, gb, first, count, nord, theta, t_prev); break;
    case 8: rc = gcp_scan_nc<8>(c, gb, first, count, nord, theta, t_prev); break;
    case 12: rc = gcp_scan_nc<12>(c, gb, first, count, nord, theta, t_prev); break;
    case 16: rc = gcp_scan_nc<16>(c, gb, first, count, nord, theta, t_prev); break;
    case 20: rc = gcp_scan_nc<20>(c, gb, first, count, nord, theta, t_prev); break;
    case 24: rc = gcp_scan_nc<24>(c, gb, first, count, nord, theta, t_prev); break;
    case 28: rc = gcp_scan_nc<28>(c, gb, first, count, nord, theta, t_prev); break;
    case 32: rc = gcp_scan_nc<32>(c, gb, first, count, nord, theta, t_prev); break;
    case 40: rc = gcp_scan_nc<40>(c, gb, first, count, nord, theta, t_prev); break;
    case 48: rc = gcp_scan_nc<48>(c, gb, first, count, nord, theta, t_prev); break;
    case 64: rc = gcp_scan_nc<64>(c, gb, first, count, nord, theta, t_prev); break;
    default: rc = gcp_scan_nc<80>(c, gb, first, count, nord, theta, t_prev); break;
    }
    if (rc)
        return rc;
    double fp_h = state_in[2 * nc2], fpp_h = state_in[2 * nc2 + 1];
    if (b->chain_host)
    {
        double* hdt = b->h_chain;  // the host's copy has the layout of this call's device arrays
        double* hA = hdt + (count + 1);
        double* hB = hA + (count + 1);
        // 24 bytes per crossing over PCIe and ~1.4 ns of host arithmetic per crossing are about the same time: the chunk
        // travels in pieces and the host walks a piece while the next ones are still on the way
        const int nsub = count >= (int64_t(1) << 17) ? lbfgsb_state::kChainPieces : 1;
        if (nsub > 1 && !b->chain_ev[0])
            for (int q = 0; q < lbfgsb_state::kChainPieces; q++)
                LBFGSX_HIP(hipEventCreateWithFlags(&b->chain_ev[q], hipEventDisableTiming));
        for (int q = 0; q < nsub; q++)
        {
            const int64_t lo = count * q / nsub, hi = count * (q + 1) / nsub;
            const int64_t dlo = q ? lo + 1 : lo;  // dt[k + 1] closes crossing k: the piece ends with dt[hi]
            if (nsub == 1)  // dt (count + 1) | A | B: contiguous, one copy
                LBFGSX_HIP(lbfgsx::copy_async(hdt, b->s_chain, sizeof(double) * 3 * size_t(count + 1), hipMemcpyDeviceToHost, c->stream));
            else
            {
                LBFGSX_HIP(lbfgsx::copy_async(hdt + dlo, b->s_fp + dlo, sizeof(double) * size_t(hi + 1 - dlo), hipMemcpyDeviceToHost, c->stream));
                LBFGSX_HIP(lbfgsx::copy_async(hA + lo, b->s_dfp + lo, sizeof(double) * size_t(hi - lo), hipMemcpyDeviceToHost, c->stream));
                LBFGSX_HIP(lbfgsx::copy_async(hB + lo, b->s_fpp + lo, sizeof(double) * size_t(hi - lo), hipMemcpyDeviceToHost, c->stream));
            }
            if (nsub > 1)
                LBFGSX_HIP(hipEventRecord(b->chain_ev[q], c->stream));
        }
        int64_t e = -1;
        for (int q = 0; q < nsub && e < 0; q++)
        {
            const int64_t lo = count * q / nsub, hi = count * (q + 1) / nsub;
            if (nsub > 1)
                LBFGSX_HIP(hipEventSynchronize(b->chain_ev[q]));
            else
                LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
            e = (c->dtype == LBFGSX_F32) ? gcp_chain_host<float>(hdt, hA, hB, lo, hi, fp_h, fpp_h)
                                         : gcp_chain_host<double>(hdt, hA, hB, lo, hi, fp_h, fpp_h);
        }
        // every copy of this chunk has landed (the walk waited for the pieces it read; the others belong to the same stream
        // and are drained by the wait below): the exit index travels through the mapped word
        *b->exit_map_host = (e >= 0) ? (unsigned long long) e : ~0ull;
        std::atomic_thread_fence(std::memory_order_release);
        switch (NC)
        {
        case 4: gcp_extract_nc<4>(c, gb, count, theta); break;
        case 8: gcp_extract_nc<8>(c, gb, count, theta); break;
        case 12: gcp_extract_nc<12>(c, gb, count, theta); break;
        case 16: gcp_extract_nc<16>(c, gb, count, theta); break;
        case 20: gcp_extract_nc<20>(c, gb, count, theta); break;
        case 24: gcp_extract_nc<24>(c, gb, count, theta); break;
        case 28: gcp_extract_nc<28>(c, gb, count, theta); break;
        case 32: gcp_extract_nc<32>(c, gb, count, theta); break;
        case 40: gcp_extract_nc<40>(c, gb, count, theta); break;
        case 48: gcp_extract_nc<48>(c, gb, count, theta); break;
        case 64: gcp_extract_nc<64>(c, gb, count, theta); break;
        default: gcp_extract_nc<80>(c, gb, count, theta); break;
        }
        LBFGSX_HIP(hipGetLastError());
    }
    double o[2 * 80 + 4];
    if (b->chain_host)
    {
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));  // k_gcp_extract's stores into the mapped block are out when the stream has drained
        for (int j = 0; j < 2 * NC + 4; j++)
            o[j] = static_cast<const volatile double*>(b->gout_host)[j];
    }
    else
    {
        const double* dout = b->s_small + (NC * NC + NC + (NC + 1) + 1 + (NC + 1));
        LBFGSX_HIP(lbfgsx::copy_async(o, dout, sizeof(double) * size_t(2 * NC + 4), hipMemcpyDeviceToHost, c->stream));
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    }
    for (int j = 0; j < nc2; j++)
    {
        state_out[j] = o[j];
        state_out[nc2 + j] = o[NC + j];
    }
    state_out[2 * nc2] = b->chain_host ? fp_h : o[2 * NC];           // f'
    state_out[2 * nc2 + 1] = b->chain_host ? fpp_h : o[2 * NC + 1];  // f''
    state_out[2 * nc2 + 2] = o[2 * NC + 2];  // break point of the last processed crossing
    *exit_at = (o[2 * NC + 3] < 0.0) ? int64_t(-1) : first + int64_t(o[2 * NC + 3]);
    return LBFGSX_OK;
}

int lbfgsx_b_cauchy_finish(lbfgsx_ctx* c, double t_cross, double tfinal, int crossed_all, int64_t* nact, int64_t* nfree)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[3] = {0, 0, -1};
    lbfgsb_state* b = c->bstate;
    const bool fuse = b->fin_fuse && c->n < (int64_t(1) << 31);
    const bool want_list = fuse && b->na_prev >= 0 && b->na_prev <= int64_t(b->na_cap);
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        b->lu_valid = false;  // the state bytes are rewritten
        b->wf_valid = false;
        lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(c->n) * (5 * sizeof(T) + 1));  // byte model: brk, x0, d read; xcp, drt and the state byte written
        LBFGSX_LAUNCH((k_cauchy_finish<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, T(t_cross), T(tfinal), crossed_all,
                           c->n, c->ws, b->dout, fuse ? P<T>(c->d) : static_cast<T*>(nullptr),
                           want_list ? b->na_list : static_cast<int*>(nullptr), b->na_cnt, b->na_cap);
    });
    LBFGSX_HIP(hipGetLastError());
    rc = fetch_doubles(c, want_list ? 3 : 2, r);
    if (rc)
        return rc;
    if (nact) *nact = int64_t(r[0]);
    if (nfree) *nfree = int64_t(r[1]);
    b->nfree_last = int64_t(r[1]);
    b->drt_ready = fuse;
    b->na_prev = int64_t(r[0]);
    b->na_n = (want_list && r[2] >= 0 && r[2] <= double(b->na_cap)) ? int64_t(r[2]) : -1;
    return LBFGSX_OK;
}

// inspection entry: the break points, vecd or the sorted row numbers as they stand; nothing of the context changes
int lbfgsx_b_cauchy_download(lbfgsx_ctx* c, int which, void* host)
{
    if (!c || !c->bstate || !host || which < LBFGSX_CV_BRK || which > LBFGSX_CV_VALS_OUT)
    {
        set_error("lbfgsx_b_cauchy_download: needs a bounded context, a LBFGSX_CV_* selector and a host pointer");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const lbfgsb_state* b = c->bstate;
    const void* dev = which == LBFGSX_CV_BRK ? b->brk : which == LBFGSX_CV_DVEC ? b->dvec : static_cast<const void*>(b->vals_out);
    const size_t bytes = size_t(c->n) * (which == LBFGSX_CV_VALS_OUT ? sizeof(int) : c->esz);
    LBFGSX_HIP(lbfgsx::copy_async(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    return LBFGSX_OK;
}

int lbfgsx_b_sub_begin(lbfgsx_ctx* c)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, false, false, /*keep_fin=*/true);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    c->bstate->sub_epoch++;
    c->bstate->wf_valid = false;  // a compact copy of the free rows belongs to one subspace minimisation
    c->bstate->wf_on = false;
    if (c->bstate->drt_ready)  // lbfgsx_b_cauchy_finish, the entry right before this one, has evaluated the statement
    {
        c->bstate->drt_ready = false;
        return LBFGSX_OK;
    }
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        lbfgsx::model_add(double(c->n) * 3 * sizeof(T));
        LBFGSX_LAUNCH((k_sub_begin<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, c->n);
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}

}  // extern "C"
