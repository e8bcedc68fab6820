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
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"

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
// the W + 1 offsets of the pack at b = vi*W (colptr has n + 1 elements, b + W <= n)
template <int W>
__device__ __forceinline__ void lin_offsets(const uint32_t* __restrict__ off, int64_t b, uint32_t (&o)[W + 1])
{
#pragma unroll
    for (int k = 0; k <= W; k++)
        o[k] = off[b + k];
}

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

// ---------------------------------------------------------------- k_eval's counterpart
// out[0] = f(x), out[1] = g.g, out[2] = x.x
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                     T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[3];
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < nv; vi += stride)
    {
        const Pack<T> px = ldv(x, vi);
        uint32_t o[W + 1];
        lin_offsets<W>(obj.colptr, vi * W, o);
        Pack<T> pg;
#pragma unroll
        for (int k = 0; k < W; k++)
            pg.e[k] = lin_coord<T>(obj, vi * W + k, px.e[k], o[k], o[k + 1], acc[0]);
        stv(g, vi, pg);
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            acc[1].add_prod(pg.e[k], pg.e[k]);
            acc[2].add_prod(px.e[k], px.e[k]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = lin_coord<T>(obj, i, x[i], obj.colptr[i], obj.colptr[i + 1], acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, gi);
            acc[2].add_prod(x[i], x[i]);
        }
    lin_row_values<T>(obj, acc[0]);
    if (grid_reduce<3>(acc, ws) && threadIdx.x == 0)
    {
        out[0] = T(acc[0].value());
        out[1] = T(acc[1].value());
        out[2] = T(acc[2].value());
    }
}

// ---------------------------------------------------------------- k_trial's counterpart
// x = xp + step*d ; g = grad f(x) ; out[0] = f(x), out[1] = g.d
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                      T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                      T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kLinTrialU;
    A acc[2];
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        Pack<T> pxp[U], pd[U];
        uint32_t o[U][W + 1];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                pxp[u] = ldv(xp, vi);
                pd[u] = ldv(d, vi);
                lin_offsets<W>(obj.colptr, vi * W, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                Pack<T> px, pg;
#pragma unroll
                for (int k = 0; k < W; k++)
                    px.e[k] = pxp[u].e[k] + step * pd[u].e[k];
#pragma unroll
                for (int k = 0; k < W; k++)
                    pg.e[k] = lin_coord<T>(obj, vi * W + k, px.e[k], o[u][k], o[u][k + 1], acc[0]);
                stv(x, vi, px);
                stv(g, vi, pg);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[1].add_prod(pg.e[k], pd[u].e[k]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T xi = xp[i] + step * d[i];
            x[i] = xi;
            const T gi = lin_coord<T>(obj, i, xi, obj.colptr[i], obj.colptr[i + 1], acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
    lin_row_values<T>(obj, acc[0]);
    if (grid_reduce<2>(acc, ws) && threadIdx.x == 0)
    {
        out[0] = T(acc[0].value());
        out[1] = T(acc[1].value());
        ws_signal(ws);
    }
}

// ---------------------------------------------------------------- k_b_eval's counterpart
// out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                       const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[2];
    double pg = 0.0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < nv; vi += stride)
    {
        const Pack<T> px = ldv(x, vi), pl = ldv(lb, vi), pu = ldv(ub, vi);
        uint32_t o[W + 1];
        lin_offsets<W>(obj.colptr, vi * W, o);
        Pack<T> pgv;
#pragma unroll
        for (int k = 0; k < W; k++)
            pgv.e[k] = lin_coord<T>(obj, vi * W + k, px.e[k], o[k], o[k + 1], acc[0]);
        stv(g, vi, pgv);
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            acc[1].add_prod(px.e[k], px.e[k]);
            pg = fmax(pg, double(projg_term(px.e[k], pgv.e[k], pl.e[k], pu.e[k])));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = lin_coord<T>(obj, i, x[i], obj.colptr[i], obj.colptr[i + 1], acc[0]);
            g[i] = gi;
            acc[1].add_prod(x[i], x[i]);
            pg = fmax(pg, double(projg_term(x[i], gi, lb[i], ub[i])));
        }
    lin_row_values<T>(obj, acc[0]);
    ext_publish<false>(pg, ws, 4);
    if (grid_reduce<2>(acc, ws))
    {
        const double pgmax = ext_collect<false>(ws, 4);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[0].value());
            out[1] = T(acc[1].value());
            out[2] = T(pgmax);
        }
    }
}

// ---------------------------------------------------------------- k_b_dg_maxstep_trial's counterpart
// out[0] = g0.d, out[1] = step_max, out[2] = f(x), out[3] = grad(x).d at x = xp + step*d
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                   const T* __restrict__ d, const T* __restrict__ lb,
                                                                   const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                   T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                   T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kLinTrialU;
    A acc[3];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        Pack<T> pxp[U], pd[U], pg0[U], plo[U], pup[U];
        uint32_t o[U][W + 1];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                pxp[u] = ldv<T>(xp, vi);
                pd[u] = ldv<T>(d, vi);
                pg0[u] = ldv<T>(g0, vi);
                plo[u] = ldv<T>(lb, vi);
                pup[u] = ldv<T>(ub, vi);
                lin_offsets<W>(obj.colptr, vi * W, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                Pack<T> px, pg;
#pragma unroll
                for (int k = 0; k < W; k++)
                {
                    px.e[k] = pxp[u].e[k] + step * pd[u].e[k];
                    acc[2].add_prod(pg0[u].e[k], pd[u].e[k]);
                    feas(pxp[u].e[k], pd[u].e[k], plo[u].e[k], pup[u].e[k]);
                }
#pragma unroll
                for (int k = 0; k < W; k++)
                    pg.e[k] = lin_coord<T>(obj, vi * W + k, px.e[k], o[u][k], o[u][k + 1], acc[0]);
                stv<T>(x, vi, px);
                stv<T>(g, vi, pg);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[1].add_prod(pg.e[k], pd[u].e[k]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            acc[2].add_prod(g0[i], d[i]);
            feas(xp[i], d[i], lb[i], ub[i]);
            const T xi = xp[i] + step * d[i];
            x[i] = xi;
            const T gi = lin_coord<T>(obj, i, xi, obj.colptr[i], obj.colptr[i + 1], acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
    lin_row_values<T>(obj, acc[0]);
    ext_publish<true>(smin, ws, 6);
    if (grid_reduce<3>(acc, ws))
    {
        const double smin_all = ext_collect<true>(ws, 6);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[2].value());
            out[1] = T(smin_all);
            out[2] = T(acc[0].value());
            out[3] = T(acc[1].value());
            ws_signal(ws);
        }
    }
}

}  // namespace lbfgsx
