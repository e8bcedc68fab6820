// lbfgspp_amd/csrc/linear_kernels.cuh -- the evaluation kernels for a LINEAR-MODEL objective
//     f(x) = sum over coordinates j of psi(x[j]; j)  +  sum over rows r of phi(z_r; r),      z = A x,
// A sparse, R x n, given in CSR (include/lbfgsx.h, "linear-model objectives").
//
// An evaluation is two launches on one stream (three when the matrix has a long column, linear_topology.hip):
//   the ROW pass   k_lin_rows / k_lin_rows_trial      z_r, then w[r] = phi'(z_r) and v[r] = phi(z_r)
//   the COLUMN pass k_lin_eval, k_lin_trial, k_lin_b_eval, k_lin_b_dg_maxstep_trial, which take the arguments of k_eval,
//                  k_trial, k_b_eval and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order,
//                  reductions and completion signal; launch_args.hpp serves all the families.
// They are compiled at run time only (jit_objective.hip): OBJ is the struct generated around the caller's two texts,
//     static constexpr bool kCoord;           T coord(const T (&x)[1], T (&g)[1], int64_t i) const;
//     T row(T z, T& dz, int64_t r) const;     and the members of LinearArgs (launch_args.hpp).
//
// Row sum.  L lanes share one row (L a power of two <= 64, fixed at bind, so a group never leaves its wavefront).  Lane l
// takes the row's entries k0+l, k0+l+L, .. in ascending order, s_l = val[k]*x[col[k]] for its first entry and
// s_l = s_l + val[k]*x[col[k]] after it; a lane with no entry holds +0.  Then s_l = s_l + s_{l+h} for l < h, h = L/2 .. 1, by
// cross-lane moves inside the group: no LDS allocation, no atomic, no reduction workspace.  z_r = s_0.  A block handles
// kBlock / L rows per step and strides over the grid.  In k_lin_rows_trial the gathered value is xp[c] + step*d[c], the
// statement c's owner executes in the column pass that follows: never a read of the x that pass writes.
//
// Gradient.  The thread that owns coordinate j writes grad[j]: psi's g[0] if there is a coordinate body, then tval[q]*w[trow[q]]
// over the entries q in [colptr[j], colptr[j+1]) of the transposed list (ascending r, the caller's order within one r),
// started from the first contribution (no leading 0 +); +0 if there is none.  A column with more than C entries is LONG: its
// chunk partials were written by k_lin_long_cols (linear_topology.hip) and the owner adds them in ascending chunk index
// instead of walking the entries.  A thread owns the W coordinates of a 16-byte pack; thread 0 of block 0 also owns the
// coordinates past the last whole pack.  Entry loads are issued in groups of kLinGroup ahead of the w gathers, the gathers
// ahead of the arithmetic.
//
// f.  The owner adds psi's value; the same launch strides over v[R] in packs and adds every row's value to the same
// order-independent accumulator (reduce.cuh).
//
// Every index read here was validated at bind: 0 <= col < n, 0 <= trow < R, list positions in [0, nnz).
#pragma once
#include "own_frame.cuh"

namespace lbfgsx {

constexpr int kLinGroup = 4;   // entries whose loads are in flight together
constexpr int kLinTrialU = 2;  // the tile depth of the two trial column kernels

// ---------------------------------------------------------------- the row pass
// ld(c) = x[c] -- from memory in k_lin_rows, recomputed from xp and d in k_lin_rows_trial
template <class T, class OBJ, class LD>
__device__ __forceinline__ void lin_rows(const OBJ& obj, LD ld)
{
    constexpr int G = kLinGroup;
    const int L = obj.L;
    const int rpb = kBlock / L;
    const int lane = int(threadIdx.x) & (L - 1);
    const int slot = int(threadIdx.x) / L;
    const int32_t* __restrict__ rowptr = obj.rowptr;
    const int32_t* __restrict__ col = obj.col;
    const T* __restrict__ val = obj.val;
    for (int64_t r0 = int64_t(blockIdx.x) * rpb; r0 < obj.R; r0 += int64_t(gridDim.x) * rpb)
    {
        const int64_t r = r0 + slot;
        const bool live = r < obj.R;
        int64_t k = 0, k1 = 0;
        if (live)
        {
            k = int64_t(rowptr[r]) + lane;
            k1 = rowptr[r + 1];
        }
        T s = T(0);
        bool has = false;
        for (; k < k1; k += int64_t(G) * L)
        {
            int32_t cj[G];
            T vj[G], xj[G];
#pragma unroll
            for (int j = 0; j < G; j++)
            {
                cj[j] = 0;
                vj[j] = T(0);
                if (k + int64_t(j) * L < k1)
                {
                    cj[j] = col[k + int64_t(j) * L];
                    vj[j] = val[k + int64_t(j) * L];
                }
            }
#pragma unroll
            for (int j = 0; j < G; j++)
            {
                xj[j] = T(0);
                if (k + int64_t(j) * L < k1)
                    xj[j] = ld(int64_t(cj[j]));
            }
#pragma unroll
            for (int j = 0; j < G; j++)
                if (k + int64_t(j) * L < k1)
                {
                    const T prod = vj[j] * xj[j];
                    s = has ? s + prod : prod;
                    has = true;
                }
        }
        // lanes l >= h compute values nobody reads; all lanes of the wavefront take part in every move
        for (int h = L >> 1; h >= 1; h >>= 1)
            s = s + __shfl_down(s, unsigned(h), L);
        if (live && lane == 0)
        {
            T dz = T(0);
            const T value = obj.row(s, dz, r);
            obj.w[r] = dz;
            obj.v[r] = value;
        }
    }
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_rows(const T* __restrict__ x, OBJ obj)
{
    lin_rows<T>(obj, [&](int64_t c) { return x[c]; });
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    lin_rows<T>(obj, [&](int64_t c) { return xp[c] + step * d[c]; });
}

// ---------------------------------------------------------------- the column pass
// coordinate j with value xj and transposed entries [lo, hi): its gradient, returned; psi's value goes to fx
template <class T, class OBJ, class A>
__device__ __forceinline__ T lin_coord(const OBJ& obj, int64_t j, T xj, uint32_t lo, uint32_t hi, A& fx)
{
    constexpr int G = kLinGroup;
    T gv = T(0);
    bool has = false;
    if (OBJ::kCoord)
    {
        const T tx[1] = {xj};
        T tg[1];
        fx.add(obj.coord(tx, tg, j));
        gv = tg[0];
        has = true;
    }
    if (hi - lo > uint32_t(obj.C))
    {
        // a long column: its slot in the (ascending) table of long columns, then its chunk partials in ascending order
        int a = 0, b = obj.nlong - 1;
        while (a < b)
        {
            const int mid = (a + b) >> 1;
            if (int64_t(obj.long_col[mid]) < j)
                a = mid + 1;
            else
                b = mid;
        }
        const T* __restrict__ part = obj.part;
        for (uint32_t q = obj.long_chunk[a]; q < obj.long_chunk[a + 1]; q++)
        {
            const T pq = part[q];
            gv = has ? gv + pq : pq;
            has = true;
        }
        return gv;
    }
    const int32_t* __restrict__ trow = obj.trow;
    const T* __restrict__ tval = obj.tval;
    const T* __restrict__ w = obj.w;
    for (int64_t q = lo; q < int64_t(hi); q += G)
    {
        int32_t rj[G];
        T vj[G], wj[G];
#pragma unroll
        for (int t = 0; t < G; t++)
        {
            rj[t] = 0;
            vj[t] = T(0);
            if (q + t < int64_t(hi))
            {
                rj[t] = trow[q + t];
                vj[t] = tval[q + t];
            }
        }
#pragma unroll
        for (int t = 0; t < G; t++)
        {
            wj[t] = T(0);
            if (q + t < int64_t(hi))
                wj[t] = w[rj[t]];
        }
#pragma unroll
        for (int t = 0; t < G; t++)
            if (q + t < int64_t(hi))
            {
                const T prod = vj[t] * wj[t];
                gv = has ? gv + prod : prod;
                has = true;
            }
    }
    return gv;
}

// every row's value, once: the launch strides over v[R] in packs; thread 0 of block 0 takes the rows past the last whole pack
template <class T, class OBJ, class A>
__device__ __forceinline__ void lin_row_values(const OBJ& obj, A& fx)
{
    constexpr int W = Vec16<T>::W;
    const T* __restrict__ v = obj.v;
    const int64_t rv = obj.R / W;
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < rv; vi += int64_t(gridDim.x) * kBlock)
    {
        const Pack<T> pv = ldv(v, vi);
#pragma unroll
        for (int k = 0; k < W; k++)
            fx.add(pv.e[k]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t r = rv * W; r < obj.R; r++)
            fx.add(v[r]);
}

// the frame's family (own_frame.cuh): n coordinates, the transposed list at colptr, and every row's value as the extra pass
struct LinFamily
{
    static constexpr int D = 1, U = kLinTrialU;
    template <class OBJ>
    static __device__ __forceinline__ int64_t nodes(const OBJ&, int64_t n)
    {
        return n;
    }
    template <class OBJ>
    static __device__ __forceinline__ const uint32_t* off(const OBJ& obj)
    {
        return obj.colptr;
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t j, const T (&xj)[1], uint32_t lo, uint32_t hi, LD, A& fx,
                                                T (&gj)[1])
    {
        gj[0] = lin_coord<T>(obj, j, xj[0], lo, hi, fx);
    }
    template <class T, class OBJ, class A>
    static __device__ __forceinline__ void extra(const OBJ& obj, A& fx)
    {
        lin_row_values<T>(obj, fx);
    }
};

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                     T* __restrict__ out)
{
    own_eval<T, LinFamily, OBJ, false>(x, g, nullptr, nullptr, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                       const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out)
{
    own_eval<T, LinFamily, OBJ, true>(x, g, lb, ub, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                      T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                      T* __restrict__ out, int rev)
{
    own_trial<T, LinFamily, OBJ, false>(xp, nullptr, d, nullptr, nullptr, step, x, g, n, obj, ws, out, rev);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                   const T* __restrict__ d, const T* __restrict__ lb,
                                                                   const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                   T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                   T* __restrict__ out, int rev)
{
    own_trial<T, LinFamily, OBJ, true>(xp, g0, d, lb, ub, step, x, g, n, obj, ws, out, rev);
}

}  // namespace lbfgsx
