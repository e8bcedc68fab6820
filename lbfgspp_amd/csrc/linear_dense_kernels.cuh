// lbfgspp_amd/csrc/linear_dense_kernels.cuh -- the evaluation kernels for a DENSE LINEAR-MODEL objective
//     f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r),      Z = A X,
// A dense, R x F, row-major with a row stride of lda >= F elements; x holds the F x D weight matrix X feature-major,
// x[j*D + c], n = F*D; D = OBJ::D is a compile-time constant of the generated struct, 1 .. 16 (include/lbfgsx.h, "dense
// linear-model objectives").  The bodies are the multi-output form's (linear_multi_kernels.cuh).
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
// Row sums.  The sparse forms' rule on the dense row: L lanes share a row (L a power of two <= 64, fixed at bind), lane l
// takes columns l, l+L, .. in ascending order, s_l[c] = A[r,k]*x[k*D + c] for its first column and s_l[c] = s_l[c] + .. after
// it, +0 without one; then s_l[c] = s_l[c] + s_{l+h}[c] for l < h, h = L/2 .. 1, by cross-lane moves: no LDS, no atomic.  The
// lanes of a row read consecutive elements of it.  linm_group<T, D>() columns are in flight together, the multi-output form's
// register reasoning for the 2*D values of the trial form.  Lane 0 runs the row body.  The same matrix given to the sparse
// forms as CSR with every entry stored, and the same L, gives the same bits.
//
// Partials.  Rows are cut into chunks of C = kDenseChunk consecutive rows (the last one shorter).  A thread owns one 16-byte
// pack of W consecutive columns and walks the rows of one chunk in ascending r with W*D accumulators, started from the first
// row's products; w[r*D ..] is the same for every thread of the chunk.  kDenseAhead rows' loads of A are in flight ahead of
// the arithmetic, 16-byte loads when the matrix base and lda allow, element loads with the same bits otherwise.  With P =
// ceil(F / W) packs, a block of kBlock threads is one chunk x kBlock packs, or, when P < kBlock, kBlock / S chunks x S packs
// with S the next power of two >= P, so a small F leaves few lanes idle.  A is read a second time here, never at a stride.
//
// Gradient.  A thread owns one 16-byte pack of consecutive coordinates (the frame's D = 1 ownership); coordinate i = j*D + c
// takes psi's g[0] if there is a coordinate body, then part[b*n + i] in ascending b, started from the first contribution,
// kLinGroup loads ahead of the adds.  Every coordinate has the same list, (0, chunks): the family's kRange.
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
// ld(j, xj) fills xj[0..D) with the weight row of feature j -- from memory in k_dense_rows, recomputed from xp and d in
// k_dense_rows_trial
template <class T, class OBJ, class LD>
__device__ __forceinline__ void dense_rows(const OBJ& obj, LD ld)
{
    constexpr int D = OBJ::D, G = linm_group<T, D>();
    const int L = obj.L;
    const int rpb = kBlock / L;
    const int lane = int(threadIdx.x) & (L - 1);
    const int slot = int(threadIdx.x) / L;
    const int64_t F = obj.F;
    for (int64_t r0 = int64_t(blockIdx.x) * rpb; r0 < obj.R; r0 += int64_t(gridDim.x) * rpb)
    {
        const int64_t r = r0 + slot;
        const bool live = r < obj.R;
        const T* __restrict__ a = obj.A + (live ? r : 0) * obj.lda;
        int64_t k = live ? lane : 0;
        const int64_t k1 = live ? F : 0;
        T s[D];
#pragma unroll
        for (int c = 0; c < D; c++)
            s[c] = T(0);
        bool has = false;
        for (; k < k1; k += int64_t(G) * L)
        {
            T vj[G], xj[G][D];
#pragma unroll
            for (int j = 0; j < G; j++)
            {
                vj[j] = T(0);
                if (k + int64_t(j) * L < k1)
                    vj[j] = a[k + int64_t(j) * L];
            }
#pragma unroll
            for (int j = 0; j < G; j++)
                if (k + int64_t(j) * L < k1)
                    ld(k + int64_t(j) * L, xj[j]);
#pragma unroll
            for (int j = 0; j < G; j++)
                if (k + int64_t(j) * L < k1)
                {
#pragma unroll
                    for (int c = 0; c < D; c++)
                    {
                        const T prod = vj[j] * xj[j][c];
                        s[c] = has ? s[c] + prod : prod;
                    }
                    has = true;
                }
        }
        // lanes l >= h compute values nobody reads; all lanes of the wavefront take part in every move
        for (int h = L >> 1; h >= 1; h >>= 1)
        {
#pragma unroll
            for (int c = 0; c < D; c++)
                s[c] = s[c] + __shfl_down(s[c], unsigned(h), L);
        }
        if (live && lane == 0)
        {
            T dz[D];
#pragma unroll
            for (int c = 0; c < D; c++)
                dz[c] = T(0);
            const T value = obj.row(s, dz, r);
#pragma unroll
            for (int c = 0; c < D; c++)
                obj.w[r * D + c] = dz[c];
            obj.v[r] = value;
        }
    }
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_rows(const T* __restrict__ x, OBJ obj)
{
    constexpr int D = OBJ::D;
    dense_rows<T>(obj, [&](int64_t j, T(&xj)[D]) __attribute__((always_inline)) { linm_load<T, D>(x + j * D, xj); });
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    constexpr int D = OBJ::D;
    dense_rows<T>(obj, [&](int64_t j, T(&xj)[D]) __attribute__((always_inline)) {
        T a[D], b[D];
        linm_load<T, D>(xp + j * D, a);
        linm_load<T, D>(d + j * D, b);
#pragma unroll
        for (int c = 0; c < D; c++)
            xj[c] = a[c] + step * b[c];
    });
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
    T gv = T(0);
    bool has = false;
    if (OBJ::kCoord)
    {
        const T tx[1] = {xi};
        T tg[1];
        fx.add(obj.coord(tx, tg, i));
        gv = tg[0];
        has = true;
    }
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
            {
                gv = has ? gv + pj[t] : pj[t];
                has = true;
            }
    }
    return gv;
}

// the frame's family (own_frame.cuh): n coordinates that all walk the chunks (0, chunks), and every row's value as the extra pass
struct DenseFamily
{
    static constexpr int D = 1, U = kLinTrialU;
    static constexpr bool kRange = true;
    template <class OBJ>
    static __device__ __forceinline__ int64_t nodes(const OBJ&, int64_t n)
    {
        return n;
    }
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
    template <class T, class OBJ, class A>
    static __device__ __forceinline__ void extra(const OBJ& obj, A& fx)
    {
        lin_row_values<T>(obj, fx);
    }
};

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out)
{
    own_eval<T, DenseFamily, OBJ, false>(x, g, nullptr, nullptr, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                         const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                         T* __restrict__ out)
{
    own_eval<T, DenseFamily, OBJ, true>(x, g, lb, ub, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                        T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                        T* __restrict__ out, int rev)
{
    own_trial<T, DenseFamily, OBJ, false>(xp, nullptr, d, nullptr, nullptr, step, x, g, n, obj, ws, out, rev);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_dense_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                     const T* __restrict__ d, const T* __restrict__ lb,
                                                                     const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                     T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                     T* __restrict__ out, int rev)
{
    own_trial<T, DenseFamily, OBJ, true>(xp, g0, d, lb, ub, step, x, g, n, obj, ws, out, rev);
}

}  // namespace lbfgsx
