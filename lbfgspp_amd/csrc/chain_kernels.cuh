// lbfgspp_amd/csrc/chain_kernels.cuh -- the four evaluation kernels for a CHAIN objective
//     f(x) = sum over t = 0 .. n-K of phi(x[t], .., x[t+K-1]; t),   K = 2 or 3,
// one term starting at every coordinate, so that neighbouring terms overlap (include/lbfgsx.h, "chain objectives").
//
// k_chain_eval, k_chain_trial, k_chain_b_eval and k_chain_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial (lbfgs_kernels.cuh, lbfgsb_kernels.cuh) and are launched with their grids: the same outputs,
// tiles, tile order, reductions and completion signal; launch_args.hpp serves both families.  They are compiled at run time
// only (jit_objective.hip): OBJ is the struct generated around the caller's text for one term,
//     static constexpr int K;   T term(const T (&x)[K], T (&g)[K], int64_t t) const;
//
// Ownership.  The thread that owns coordinate j writes grad[j] and adds the value of the term that STARTS at j (if one
// does: j <= n-K) to f's accumulator, once.  grad[j] is the sum of g_t[j-t] over t = max(0, j-K+1) .. min(j, n-K) in
// ascending t, started from the first contribution (no leading 0 +).  A thread owns the W coordinates of a 16-byte pack
// [b, b+W); thread 0 of block 0 also owns the coordinates past the last whole pack.  So a thread evaluates the terms that
// start at b-(K-1) .. b+W-1, clipped to [0, n-K], from a window of W + 2(K-1) values of x.
//
// The window.  In all four kernels adjacent lanes hold adjacent packs, so the K-1 values on either side come from the
// neighbouring lanes by cross-lane moves, which run with all 64 lanes of the wave in the loop (the loops below run on the
// wave's first pack, not the lane's).  Only a lane without a neighbour reads memory: lane 0 of a wave to its left, lane 63
// and the lane that holds the last whole pack to their right (there the halo may be tail coordinates).  Those reads are
// issued with the pack's own loads.  In the trial kernels a halo value is the neighbour's computed xp + step*d or the same
// statement on halo loads of xp and d -- never a read of the x this launch writes.
// No index below 0 or at or above n is loaded, and a term that does not lie inside [0, n) is not evaluated, so the text of a
// term may read p0[i] .. p0[i+K-1].
#pragma once
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"

namespace lbfgsx {

// The coordinate whose value slot j of a lane's spare halo registers holds, or -1: lane 0 fetches x[b-H+j], another lane
// without a right neighbour x[b+W+j]; lane 0 without a right neighbour fetches that side when the window is put together
// (chain_window's `late`)
template <class T, int K>
__device__ __forceinline__ int64_t chain_edge_index(int64_t vi, int64_t nv, int64_t n, int j)
{
    constexpr int W = Vec16<T>::W, H = K - 1;
    const int lane = threadIdx.x & 63;
    if (vi >= nv)
        return -1;
    int64_t idx = -1;
    if (lane == 0)
        idx = vi * W - H + j;
    else if (lane == 63 || vi + 1 >= nv)
        idx = vi * W + W + j;
    return (idx >= 0 && idx < n) ? idx : -1;
}

// xw[0 .. W+2H) = x[b-H .. b+W+H) around the pack px at vi.  Called by all 64 lanes of the wave, whether they hold a pack
// or not (a lane past the end hands its neighbour values nobody uses).  edge: the values at chain_edge_index's coordinates
// (anything where it said -1: the terms that would read them are not evaluated); late(j): x[b+W+j] from memory, or anything
// when that coordinate is not below n.
template <class T, int K, class LATE>
__device__ __forceinline__ void chain_window(const Pack<T>& px, const T (&edge)[K - 1], int64_t vi, int64_t nv, LATE late,
                                             T (&xw)[Vec16<T>::W + 2 * (K - 1)])
{
    constexpr int W = Vec16<T>::W, H = K - 1;
    static_assert(H >= 1 && H <= W, "the halo of a pack lies inside the neighbouring pack");
    const int lane = threadIdx.x & 63;
    const bool mem_r = lane == 63 || vi + 1 >= nv;
#pragma unroll
    for (int j = 0; j < H; j++)
    {
        const T up = __shfl_up(px.e[W - H + j], 1, 64);
        const T dn = __shfl_down(px.e[j], 1, 64);
        xw[j] = (lane == 0) ? edge[j] : up;
        xw[H + W + j] = mem_r ? edge[j] : dn;
    }
    if (lane == 0 && mem_r && vi < nv)
    {
#pragma unroll
        for (int j = 0; j < H; j++)
            xw[H + W + j] = late(j);
    }
#pragma unroll
    for (int k = 0; k < W; k++)
        xw[H + k] = px.e[k];
}

// the terms of one pack from its window: gradient of the pack's W coordinates, values of the terms that start inside it.
// ALL: every term b-H .. b+W-1 exists (a pack away from both ends of x)
template <bool ALL, class T, class OBJ, class A>
__device__ __forceinline__ void chain_terms(const OBJ& obj, int64_t b, int64_t n, const T (&xw)[Vec16<T>::W + 2 * (OBJ::K - 1)],
                                            Pack<T>& g, A& fx)
{
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    bool has[W];
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        has[k] = false;
        g.e[k] = T(0);
    }
#pragma unroll
    for (int s = 0; s < W + H; s++)
    {
        const int64_t t = b - H + s;
        if (ALL || (t >= 0 && t + K <= n))
        {
            T tx[K], tg[K];
#pragma unroll
            for (int j = 0; j < K; j++)
                tx[j] = xw[s + j];
            const T v = obj.term(tx, tg, t);
#pragma unroll
            for (int j = K - 1; j >= 0; j--)
            {
                const int k = s + j - H;  // the pack's coordinate that tg[j] belongs to
                if (k >= 0 && k < W)
                {
                    g.e[k] = has[k] ? g.e[k] + tg[j] : tg[j];
                    has[k] = true;
                }
            }
            if (s >= H)
                fx.add(v);
        }
    }
}

template <class T, class OBJ, class A>
__device__ __forceinline__ void chain_pack(const OBJ& obj, int64_t vi, int64_t n, const T (&xw)[Vec16<T>::W + 2 * (OBJ::K - 1)],
                                           Pack<T>& g, A& fx)
{
    constexpr int W = Vec16<T>::W, H = OBJ::K - 1;
    const int64_t b = vi * W;
    if (b >= H && b + W + H <= n)
        chain_terms<true>(obj, b, n, xw, g, fx);
    else
        chain_terms<false>(obj, b, n, xw, g, fx);
}

// a coordinate past the last whole pack (thread 0 of block 0): its gradient, returned, and the value of the term that starts
// there.  ld(k) = x[k] for k in [0, n) -- from memory in the evaluation kernels, recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T chain_tail(const OBJ& obj, int64_t i, int64_t n, LD ld, A& fx)
{
    constexpr int K = OBJ::K;
    T gi = T(0);
    bool has = false;
#pragma unroll
    for (int o = K - 1; o >= 0; o--)  // the term that starts o coordinates before i: ascending t
    {
        const int64_t t = i - o;
        if (t >= 0 && t + K <= n)
        {
            T tx[K], tg[K];
#pragma unroll
            for (int j = 0; j < K; j++)
                tx[j] = ld(t + j);
            const T v = obj.term(tx, tg, t);
            gi = has ? gi + tg[o] : tg[o];
            has = true;
            if (o == 0)
                fx.add(v);
        }
    }
    return gi;
}

// ---------------------------------------------------------------- k_eval's counterpart
// out[0] = f(x), out[1] = g.g, out[2] = x.x
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_chain_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj,
                                                       RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    A acc[3];
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        Pack<T> px;
        T edge[H], xw[W + 2 * H];
#pragma unroll
        for (int k = 0; k < W; k++)
            px.e[k] = T(0);
        if (vi < nv)
            px = ldv(x, vi);
#pragma unroll
        for (int j = 0; j < H; j++)
        {
            const int64_t e = chain_edge_index<T, K>(vi, nv, n, j);
            edge[j] = T(0);
            if (e >= 0)
                edge[j] = x[e];
        }
        chain_window<T, K>(px, edge, vi, nv, [&](int j) { return (vi * W + W + j < n) ? x[vi * W + W + j] : T(0); }, xw);
        if (vi < nv)
        {
            Pack<T> pg;
            chain_pack(obj, vi, n, xw, pg, acc[0]);
            stv(g, vi, pg);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[1].add_prod(pg.e[k], pg.e[k]);
                acc[2].add_prod(px.e[k], px.e[k]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = chain_tail<T>(obj, i, n, [&](int64_t k) { return x[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, gi);
            acc[2].add_prod(x[i], x[i]);
        }
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
__global__ void __launch_bounds__(kBlock) k_chain_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                        T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj,
                                                        RedWs ws, T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    constexpr int U = 4;
    A acc[2];
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)  // the block's: all lanes stay in
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        Pack<T> pxp[U], pd[U];
        T exp_[U][H], ed[U][H];  // the halo this lane has no neighbour for: xp and d there
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
#pragma unroll
            for (int k = 0; k < W; k++)
                pxp[u].e[k] = pd[u].e[k] = T(0);
            if (vi < nv)
            {
                pxp[u] = ldv(xp, vi);
                pd[u] = ldv(d, vi);
            }
#pragma unroll
            for (int j = 0; j < H; j++)
            {
                const int64_t e = chain_edge_index<T, K>(vi, nv, n, j);
                exp_[u][j] = ed[u][j] = T(0);
                if (e >= 0)
                {
                    exp_[u][j] = xp[e];
                    ed[u][j] = d[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            Pack<T> px;
            T edge[H], xw[W + 2 * H];
#pragma unroll
            for (int k = 0; k < W; k++)
                px.e[k] = pxp[u].e[k] + step * pd[u].e[k];
#pragma unroll
            for (int j = 0; j < H; j++)
                edge[j] = exp_[u][j] + step * ed[u][j];
            chain_window<T, K>(px, edge, vi, nv,
                               [&](int j) {
                                   const int64_t e = vi * W + W + j;
                                   return (e < n) ? xp[e] + step * d[e] : T(0);
                               },
                               xw);
            if (vi < nv)
            {
                Pack<T> pg;
                chain_pack(obj, vi, n, xw, pg, acc[0]);
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
            x[i] = xp[i] + step * d[i];
            const T gi = chain_tail<T>(obj, i, n, [&](int64_t k) { return xp[k] + step * d[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
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
__global__ void __launch_bounds__(kBlock) k_chain_b_eval(const T* __restrict__ x, T* __restrict__ g,
                                                         const T* __restrict__ lb, const T* __restrict__ ub, int64_t n,
                                                         OBJ obj, RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    A acc[2];
    double pg = 0.0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        Pack<T> px, pl, pu;
        T edge[H], xw[W + 2 * H];
#pragma unroll
        for (int k = 0; k < W; k++)
            px.e[k] = T(0);
        if (vi < nv)
        {
            px = ldv(x, vi);
            pl = ldv(lb, vi);
            pu = ldv(ub, vi);
        }
#pragma unroll
        for (int j = 0; j < H; j++)
        {
            const int64_t e = chain_edge_index<T, K>(vi, nv, n, j);
            edge[j] = T(0);
            if (e >= 0)
                edge[j] = x[e];
        }
        chain_window<T, K>(px, edge, vi, nv, [&](int j) { return (vi * W + W + j < n) ? x[vi * W + W + j] : T(0); }, xw);
        if (vi < nv)
        {
            Pack<T> pgv;
            chain_pack(obj, vi, n, xw, pgv, acc[0]);
            stv(g, vi, pgv);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[1].add_prod(px.e[k], px.e[k]);
                pg = fmax(pg, double(projg_term(px.e[k], pgv.e[k], pl.e[k], pu.e[k])));
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = chain_tail<T>(obj, i, n, [&](int64_t k) { return x[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(x[i], x[i]);
            pg = fmax(pg, double(projg_term(x[i], gi, lb[i], ub[i])));
        }
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
__global__ void __launch_bounds__(kBlock) k_chain_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                     const T* __restrict__ d, const T* __restrict__ lb,
                                                                     const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                     T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                     T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    constexpr int U = 4;
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
        T exp_[U][H], ed[U][H];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
#pragma unroll
            for (int k = 0; k < W; k++)
                pxp[u].e[k] = pd[u].e[k] = T(0);
            if (vi < nv)
            {
                pxp[u] = ldv<T>(xp, vi);
                pd[u] = ldv<T>(d, vi);
                pg0[u] = ldv<T>(g0, vi);
                plo[u] = ldv<T>(lb, vi);
                pup[u] = ldv<T>(ub, vi);
            }
#pragma unroll
            for (int j = 0; j < H; j++)
            {
                const int64_t e = chain_edge_index<T, K>(vi, nv, n, j);
                exp_[u][j] = ed[u][j] = T(0);
                if (e >= 0)
                {
                    exp_[u][j] = xp[e];
                    ed[u][j] = d[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            Pack<T> px;
            T edge[H], xw[W + 2 * H];
#pragma unroll
            for (int k = 0; k < W; k++)
                px.e[k] = pxp[u].e[k] + step * pd[u].e[k];
#pragma unroll
            for (int j = 0; j < H; j++)
                edge[j] = exp_[u][j] + step * ed[u][j];
            chain_window<T, K>(px, edge, vi, nv,
                               [&](int j) {
                                   const int64_t e = vi * W + W + j;
                                   return (e < n) ? xp[e] + step * d[e] : T(0);
                               },
                               xw);
            if (vi < nv)
            {
                Pack<T> pg;
#pragma unroll
                for (int k = 0; k < W; k++)
                {
                    acc[2].add_prod(pg0[u].e[k], pd[u].e[k]);
                    feas(pxp[u].e[k], pd[u].e[k], plo[u].e[k], pup[u].e[k]);
                }
                chain_pack(obj, vi, n, xw, pg, acc[0]);
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
            x[i] = xp[i] + step * d[i];
            const T gi = chain_tail<T>(obj, i, n, [&](int64_t k) { return xp[k] + step * d[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
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
