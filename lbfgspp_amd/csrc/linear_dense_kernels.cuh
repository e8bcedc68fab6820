// lbfgspp_amd/csrc/linear_dense_kernels.cuh -- the evaluation kernels for a DENSE LINEAR-MODEL objective
//     f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r),      Z = A X,
// A dense, R x F, row-major with a row stride of lda >= F elements; x holds the F x D weight matrix X feature-major,
// x[j*D + c], n = F*D; D = OBJ::D is a compile-time constant of the generated struct, 1 .. 16 (include/lbfgsx.h, "dense
// linear-model objectives").  The bodies are the multi-output form's (linear_multi_kernels.cuh), and the row pass is the
// sparse forms' own (lin_rows, linear_kernels.cuh) over the dense row as its entry source (LinDense).
//
// An evaluation is three launches on one stream, no host wait in between:
//   the ROW pass     k_dense_rows / k_dense_rows_trial   Z[r, :], then w[r*D + c] = dphi/dz_c and v[r] = phi
//   the PARTIAL pass k_dense_partials                    part[b*n + j*D + c] = sum over the rows r of chunk b of A[r,j]*w[r*D+c]
//   the COLUMN pass  k_dense_eval, k_dense_trial, k_dense_b_eval, k_dense_b_dg_maxstep_trial: own_eval / own_trial
//                    (own_frame.cuh) with the arguments, grids, tile order, reductions and completion signal of k_eval, k_trial,
//                    k_b_eval and k_b_dg_maxstep_trial.
// OBJ is the struct generated around the caller's two texts,
//     static constexpr int D;  static constexpr bool kCoord;   T coord(const T (&x)[1], T (&g)[1], int64_t i) const;
//     T row(const T (&z)[D], T (&dz)[D], int64_t r) const;      and the members of DenseArgs (launch_args.hpp).
// k_dense_partials holds no caller text; it is instantiated in the generated unit all the same, so that D stays a
// compile-time constant without a precompiled copy per (T, D).
//
// Row sums.  lin_rows on the dense row: L lanes share a row (L a power of two <= 64, fixed at bind), lane l takes columns
// l, l+L, .. in ascending order, every column an entry (k, A[r,k]); the lanes of a row read consecutive elements of it.  The
// statements being the sparse forms', the same matrix given to them as CSR with every entry stored, and the same L, gives
// the same bits.
//
// Partials.  Rows are cut into chunks of C = kDenseChunk consecutive rows (the last one shorter).  A thread owns one 16-byte
// pack of W consecutive columns and walks the rows of one chunk in ascending r with W*D accumulators, started from the first
// row's products; w[r*D ..] is the same for every thread of the chunk.  kDenseAhead rows' loads of A are in flight ahead of
// the arithmetic, 16-byte loads when the matrix base and lda allow, element loads with the same bits otherwise.  With P =
// ceil(F / W) packs, a block of kBlock threads is one chunk x kBlock packs, or, when P < kBlock, kBlock / S chunks x S packs
// with S the next power of two >= P, so a small F leaves few lanes idle.  A is read a second time here, never at a stride.
//
// Gradient.  A thread owns one 16-byte pack of consecutive coordinates (the frame's D = 1 ownership); coordinate i = j*D + c
// takes psi's g[0] if there is a coordinate body (lin_coord_start, as in the sparse forms), then part[b*n + i] in ascending b,
// started from the first contribution, kLinGroup loads ahead of the adds.  Every coordinate has the same list, (0, chunks): the family's kRange.
//
// f.  As the sparse forms: psi's values by the owners, and every row's value from v[R] by the same launch.
//
// Bounds.  R >= 1, F >= 1, lda >= F and chunks = ceil(R / C) were checked at bind; w has R*D elements, v has R, part has
// chunks*n.  Every read of A is at r*lda + j with r < R and j < F.
#pragma once
#include "linear_multi_kernels.cuh"

namespace lbfgsx {

constexpr int kDenseAhead = 4;  // rows whose loads of A are in flight together in the partial pass

// ---------------------------------------------------------------- the row pass
// the entry source of a dense matrix (lin_rows, linear_kernels.cuh): lane `lane` of a live row starts at column `lane` and
// the row ends before F; entry k of the row is (k, A[r*lda + k]), read only if it is `in` the row
template <class T>
struct LinDense
{
    typedef int64_t col_t;
    const T* __restrict__ A;
    const T* __restrict__ row;
    int64_t F, lda;
    template <class OBJ>
    __device__ __forceinline__ explicit LinDense(const OBJ& obj) : A(obj.A), row(obj.A), F(obj.F), lda(obj.lda)
    {
    }
    __device__ __forceinline__ void span(int64_t r, bool live, int lane, int64_t& k, int64_t& k1)
    {
        row = A + (live ? r : 0) * lda;
        k = live ? lane : 0;
        k1 = live ? F : 0;
    }
    __device__ __forceinline__ void entry(int64_t k, bool in, col_t& c, T& v) const
    {
        c = k;
        v = T(0);
        if (in)
            v = row[k];
    }
};

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_rows(const T* __restrict__ x, OBJ obj)
{
    lin_rows<T, LinDense<T>>(obj, LinGather<T, OBJ::D>{x});
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    lin_rows<T, LinDense<T>>(obj, LinGatherTrial<T, OBJ::D>{xp, d, step});
}

// ---------------------------------------------------------------- the partial pass
// the slot width of a block: kBlock packs, or the next power of two >= packs when that is smaller.  The work items of the
// pass are groups of kBlock / S chunks x blocks of S packs (launch_args.hpp: dense_partials_grid counts them for the launch)
__device__ __forceinline__ int dense_slot(int64_t packs)
{
    int S = 1;
    while (S < kBlock && int64_t(S) < packs)
        S *= 2;
    return S;
}

// the W values of A at row r, columns j0 .. j0+W-1 (nv of them exist): a 16-byte load when `vec`, element loads otherwise
template <class T>
__device__ __forceinline__ Pack<T> dense_load(const T* __restrict__ A, int64_t lda, int64_t r, int64_t j0, int nv, bool vec)
{
    constexpr int W = Vec16<T>::W;
    Pack<T> p;
    if (vec)
        p = ldv(A + r * lda, j0 / W);
    else
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            p.e[k] = k < nv ? A[r * lda + j0 + k] : T(0);
    }
    return p;
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_partials(OBJ obj)
{
    constexpr int W = Vec16<T>::W, D = OBJ::D, G = kDenseAhead;
    const int64_t F = obj.F, R = obj.R, lda = obj.lda, n = F * D;
    const int64_t packs = (F + W - 1) / W;
    const int S = dense_slot(packs);
    const int cpb = kBlock / S;
    const int64_t pblocks = (packs + S - 1) / S;
    const int64_t items = ((obj.chunks + cpb - 1) / cpb) * pblocks;
    const T* __restrict__ A = obj.A;
    const T* __restrict__ w = obj.w;
    T* __restrict__ part = obj.part;
    // 16-byte loads need every row's base on a 16-byte boundary
    const bool aligned = (reinterpret_cast<unsigned long long>(A) % 16 == 0) && ((lda * int64_t(sizeof(T))) % 16 == 0);
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
    {
        const int64_t b = (item / pblocks) * cpb + int(threadIdx.x) / S;
        const int64_t pk = (item % pblocks) * S + (int(threadIdx.x) & (S - 1));
        const int64_t j0 = pk * W;
        if (b >= obj.chunks || j0 >= F)
            continue;
        const int nv = int(F - j0 < W ? F - j0 : W);
        const bool vec = aligned && nv == W;
        const int64_t ra = b * obj.C, rb = (ra + obj.C < R) ? ra + obj.C : R;
        T acc[W][D];
        {
            const Pack<T> a0 = dense_load<T>(A, lda, ra, j0, nv, vec);
            T w0[D];
            linm_load<T, D>(w + ra * D, w0);
#pragma unroll
            for (int k = 0; k < W; k++)
#pragma unroll
                for (int c = 0; c < D; c++)
                    acc[k][c] = a0.e[k] * w0[c];
        }
        for (int64_t r = ra + 1; r < rb; r += G)
        {
            Pack<T> ar[G];
#pragma unroll
            for (int t = 0; t < G; t++)
                if (r + t < rb)
                    ar[t] = dense_load<T>(A, lda, r + t, j0, nv, vec);
#pragma unroll
            for (int t = 0; t < G; t++)
                if (r + t < rb)
                {
                    T wr[D];
                    linm_load<T, D>(w + (r + t) * D, wr);
#pragma unroll
                    for (int k = 0; k < W; k++)
#pragma unroll
                        for (int c = 0; c < D; c++)
                            acc[k][c] = acc[k][c] + ar[t].e[k] * wr[c];
                }
        }
        T* __restrict__ out = part + b * n + j0 * D;
#pragma unroll
        for (int k = 0; k < W; k++)
            if (k < nv)
            {
#pragma unroll
                for (int c = 0; c < D; c++)
                    out[k * D + c] = acc[k][c];
            }
    }
}

// ---------------------------------------------------------------- the column pass
// coordinate i with value xi: its gradient, returned; psi's value goes to fx.  The partials of chunks [lo, hi) in ascending
// order, kLinGroup loads ahead of the adds
template <class T, class OBJ, class A>
__device__ __forceinline__ T dense_coord(const OBJ& obj, int64_t i, T xi, uint32_t lo, uint32_t hi, A& fx)
{
    constexpr int G = kLinGroup;
    const int64_t n = obj.F * OBJ::D;
    LinSum<T> gv = lin_coord_start<T>(obj, i, xi, fx);
    const T* __restrict__ part = obj.part;
    for (int64_t q = lo; q < int64_t(hi); q += G)
    {
        T pj[G];
#pragma unroll
        for (int t = 0; t < G; t++)
        {
            pj[t] = T(0);
            if (q + t < int64_t(hi))
                pj[t] = part[(q + t) * n + i];
        }
#pragma unroll
        for (int t = 0; t < G; t++)
            if (q + t < int64_t(hi))
                gv.add(pj[t]);
    }
    return gv.value;
}

// the frame's family (own_frame.cuh): n coordinates that all walk the chunks (0, chunks)
struct DenseFamily : LinFamilyBase
{
    static constexpr bool kRange = true;
    template <class OBJ>
    static __device__ __forceinline__ void range(const OBJ& obj, int64_t, uint32_t& lo, uint32_t& hi)
    {
        lo = 0u;
        hi = uint32_t(obj.chunks);
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t i, const T (&xi)[1], uint32_t lo, uint32_t hi, LD, A& fx,
                                                T (&gi)[1])
    {
        gi[0] = dense_coord<T>(obj, i, xi[0], lo, hi, fx);
    }
};

// k_dense_eval, k_dense_trial, k_dense_b_eval, k_dense_b_dg_maxstep_trial
LBFGSX_OWN_KERNELS(k_dense, DenseFamily)

}  // namespace lbfgsx
