// lbfgspp_amd/csrc/graph_kernels.cuh -- the four evaluation kernels for a GRAPH objective
//     f(x) = sum over nodes v of psi(x[v]; v)  +  sum over edges e of phi(x[ei[e]], x[ej[e]]; e),
// x of n coordinates (the nodes), E edges given as an index list (include/lbfgsx.h, "graph objectives").
//
// k_graph_eval, k_graph_trial, k_graph_b_eval and k_graph_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion
// signal; launch_args.hpp serves all four families.  They are compiled at run time only (jit_objective.hip): OBJ is the
// struct generated around the caller's two texts,
//     static constexpr bool kNode;            T node(const T (&x)[1], T (&g)[1], int64_t i) const;
//     const uint32_t* off; const GraphEntry* inc; int64_t E;
//     T edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j) const;
//
// The incidence list (graph_topology.hip, built on the device at bind from validated indices).  The entries of node v are
// inc[off[v] .. off[v+1]), in ascending edge index e; an entry is 8 bytes, {other, (e << 1) | side}: v is end `side` of edge
// e (0: ei[e], 1: ej[e]) and `other` is the edge's other end.
//
// Ownership.  The thread that owns coordinate v writes grad[v]: psi's g[0] if there is a node term, then g_e[side] of v's
// entries in list order, started from the first contribution (no leading 0 +); +0 if there is none.  It adds psi's value to
// f's accumulator, and an edge's value when v is the edge's end 0.  So an edge's term is evaluated twice, once from each
// end, on identical inputs (x[ei[e]], x[ej[e]], e, ei[e], ej[e]) by the same instructions: both evaluations have the same
// bits, and no float atomic is needed.  A thread owns the W coordinates of a 16-byte pack; thread 0 of block 0 also owns the
// coordinates past the last whole pack.
//
// The walk.  Per owned node: two offsets, then groups of kGraphGroup entries -- the group's entry loads are issued before
// its gathers, the gathers before its terms -- so that a group costs two memory latencies instead of 2*kGraphGroup.  In the
// trial kernels a gathered value is xp[u] + step*d[u], the statement u's owner executes: never a read of the x this launch
// writes.  Every index read from the list was validated at bind (0 <= other < n, other != v), every list position lies in
// [0, 2E).
#pragma once
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"
#include "graph_entry.hpp"

namespace lbfgsx {

constexpr int kGraphGroup = 4;   // entries whose loads are in flight together
constexpr int kGraphTrialU = 2;  // the tile depth of the two trial kernels

// the W + 1 offsets of the pack at b = vi*W (off has n + 1 elements, b + W <= n)
template <int W>
__device__ __forceinline__ void graph_offsets(const uint32_t* __restrict__ off, int64_t b, uint32_t (&o)[W + 1])
{
#pragma unroll
    for (int k = 0; k <= W; k++)
        o[k] = off[b + k];
}

// node v with value xv and entries [lo, hi): its gradient, returned; its node value and the values of the edges it is end 0
// of go to fx.  ld(u) = x[u] -- from memory in the evaluation kernels, recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T graph_node(const OBJ& obj, int64_t v, T xv, uint32_t lo, uint32_t hi, LD ld, A& fx)
{
    constexpr int G = kGraphGroup;
    T gv = T(0);
    bool has = false;
    if (OBJ::kNode)
    {
        const T tx[1] = {xv};
        T tg[1];
        fx.add(obj.node(tx, tg, v));
        gv = tg[0];
        has = true;
    }
    const GraphEntry* __restrict__ inc = obj.inc;
    for (int64_t q = lo; q < int64_t(hi); q += G)
    {
        GraphEntry en[G];
        T xo[G];
#pragma unroll
        for (int j = 0; j < G; j++)
        {
            en[j].other = 0;
            en[j].es = 0;
            if (q + j < int64_t(hi))
                en[j] = inc[q + j];
        }
#pragma unroll
        for (int j = 0; j < G; j++)
        {
            xo[j] = T(0);
            if (q + j < int64_t(hi))
                xo[j] = ld(int64_t(en[j].other));
        }
#pragma unroll
        for (int j = 0; j < G; j++)
            if (q + j < int64_t(hi))
            {
                const bool far = (en[j].es & 1u) != 0;  // v is the edge's end 1
                const int64_t u = en[j].other;
                const T tx[2] = {far ? xo[j] : xv, far ? xv : xo[j]};
                T tg[2];
                const T val = obj.edge(tx, tg, int64_t(en[j].es >> 1), far ? u : v, far ? v : u);
                const T mine = far ? tg[1] : tg[0];
                gv = has ? gv + mine : mine;
                has = true;
                if (!far)
                    fx.add(val);
            }
    }
    return gv;
}

// ---------------------------------------------------------------- k_eval's counterpart
// out[0] = f(x), out[1] = g.g, out[2] = x.x
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_graph_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj,
                                                       RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[3];
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    auto ld = [&](int64_t u) { return x[u]; };
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < nv; vi += stride)
    {
        const Pack<T> px = ldv(x, vi);
        uint32_t o[W + 1];
        graph_offsets<W>(obj.off, vi * W, o);
        Pack<T> pg;
#pragma unroll
        for (int k = 0; k < W; k++)
            pg.e[k] = graph_node<T>(obj, vi * W + k, px.e[k], o[k], o[k + 1], ld, acc[0]);
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
            const T gi = graph_node<T>(obj, i, x[i], obj.off[i], obj.off[i + 1], ld, acc[0]);
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
__global__ void __launch_bounds__(kBlock) k_graph_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                        T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                        T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kGraphTrialU;
    A acc[2];
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    auto ld = [&](int64_t u) { return xp[u] + step * d[u]; };
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
                graph_offsets<W>(obj.off, vi * W, o[u]);
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
                    pg.e[k] = graph_node<T>(obj, vi * W + k, px.e[k], o[u][k], o[u][k + 1], ld, acc[0]);
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
            const T gi = graph_node<T>(obj, i, xi, obj.off[i], obj.off[i + 1], ld, acc[0]);
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
__global__ void __launch_bounds__(kBlock) k_graph_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                         const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                         T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[2];
    double pg = 0.0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    auto ld = [&](int64_t u) { return x[u]; };
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < nv; vi += stride)
    {
        const Pack<T> px = ldv(x, vi), pl = ldv(lb, vi), pu = ldv(ub, vi);
        uint32_t o[W + 1];
        graph_offsets<W>(obj.off, vi * W, o);
        Pack<T> pgv;
#pragma unroll
        for (int k = 0; k < W; k++)
            pgv.e[k] = graph_node<T>(obj, vi * W + k, px.e[k], o[k], o[k + 1], ld, acc[0]);
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
            const T gi = graph_node<T>(obj, i, x[i], obj.off[i], obj.off[i + 1], ld, acc[0]);
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
__global__ void __launch_bounds__(kBlock) k_graph_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                     const T* __restrict__ d, const T* __restrict__ lb,
                                                                     const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                     T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                     T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kGraphTrialU;
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
    auto ld = [&](int64_t u) { return xp[u] + step * d[u]; };
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
                graph_offsets<W>(obj.off, vi * W, o[u]);
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
                    pg.e[k] = graph_node<T>(obj, vi * W + k, px.e[k], o[u][k], o[u][k + 1], ld, acc[0]);
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
            const T gi = graph_node<T>(obj, i, xi, obj.off[i], obj.off[i + 1], ld, acc[0]);
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
