// lbfgspp_amd/csrc/own_frame.cuh -- the frame of the owner-computes gather kernels: the four evaluation kernels of a GRAPH,
// a MESH and a LINEAR-MODEL objective (graph_kernels.cuh, mesh_kernels.cuh, the column pass of linear_kernels.cuh,
// linear_multi_kernels.cuh, linear_dense_kernels.cuh and linear_graph_kernels.cuh) are own_eval and own_trial, bounded or
// not, around the family's walk of one node's list.  LBFGSX_OWN_KERNELS, at the end of this file, defines a family's four
// kernels.
//
// Ownership.  x holds D unknowns per node, node-major.  A thread owns W = 16 / sizeof(T) consecutive nodes: exactly D whole
// 16-byte packs of x from pack vi*D; it loads the W + 1 offsets of its nodes' lists, walks each list and writes the nodes'
// D packs of grad (and of x in the trial kernels).  Thread 0 of block 0 also owns the trailing nodes past the last whole
// group, one at a time.  The sums go into the reductions of k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial, with their
// outputs, tile order and completion signal.
//
// A family F supplies what differs:
//     static constexpr int D = unknowns per node;  U = the tile depth of the two trial kernels
//     int64_t nodes(const OBJ&, int64_t n)                      the nodes of a problem of n unknowns
//     const uint32_t* off(const OBJ&)                           the offsets of the nodes' lists, nodes + 1 of them
//     or  static constexpr bool kRange = true;  void range(obj, v, lo, hi)   a family whose nodes share lists (the multi-output
//                                                               linear model: D coordinates walk one feature's list): node
//                                                               v's entries [lo, hi), in place of off[v] and off[v + 1];
//                                                               kRange = false is the same as no kRange
//     void node<T>(obj, v, xv[D], lo, hi, ld, fx, gv[D])        node v with values xv and entries [lo, hi): its D partial
//                                                               derivatives to gv, what it owns of f to fx; ld(i) = x[i]
//     void extra<T>(obj, fx)                                    what else the launch adds to f, after the tail
#pragma once
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"
#include "frame_kernels.cuh"

namespace lbfgsx {

// a sum in a fixed order that starts from its first term (no leading 0 +); +0 without one: what a node's walk accumulates
// its partial derivative in, whichever family's lists it walks
template <class T>
struct LinSum
{
    T value = T(0);
    bool has = false;
    __device__ __forceinline__ void add(T t)
    {
        value = has ? value + t : t;
        has = true;
    }
};

// does family F give a node's (lo, hi) itself (F::kRange); the default is the load from F::off
template <class F, class = void>
struct OwnRange
{
    static constexpr bool value = false;
};
template <class F>
struct OwnRange<F, decltype(void(F::kRange))>
{
    static constexpr bool value = F::kRange;
};
// the offsets a thread holds for its W nodes: W + 1 consecutive ones, or a (lo, hi) pair per node
template <class F, int W>
constexpr int own_noff = OwnRange<F>::value ? 2 * W : W + 1;

// the offsets of the node group at b = vi*W (off has nodes + 1 elements, b + W <= nodes): node k's entries are
// [o[k], o[k + 1]), or [o[2k], o[2k + 1]) from F::range
template <class F, int W, class OBJ>
__device__ __forceinline__ void own_offsets(const OBJ& obj, int64_t b, uint32_t (&o)[own_noff<F, W>])
{
    if constexpr (OwnRange<F>::value)
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            F::range(obj, b + k, o[2 * k], o[2 * k + 1]);
    }
    else
    {
        const uint32_t* __restrict__ off = F::off(obj);
#pragma unroll
        for (int k = 0; k <= W; k++)
            o[k] = off[b + k];
    }
}

// the W nodes of group vi: their values from the D packs px, their gradients into the D packs pg
template <class T, class F, class OBJ, class LD, class A>
__device__ __forceinline__ void own_group_nodes(const OBJ& obj, int64_t vi, const Pack<T> (&px)[F::D],
                                                const uint32_t (&o)[own_noff<F, Vec16<T>::W>], LD ld, A& fx,
                                                Pack<T> (&pg)[F::D])
{
    constexpr int W = Vec16<T>::W, D = F::D;
    constexpr int S = OwnRange<F>::value ? 2 : 1;  // o's stride from one node to the next
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        T xv[D], gv[D];
#pragma unroll
        for (int d = 0; d < D; d++)
            xv[d] = px[(k * D + d) / W].e[(k * D + d) % W];
        F::template node<T>(obj, vi * W + k, xv, o[S * k], o[S * k + 1], ld, fx, gv);
#pragma unroll
        for (int d = 0; d < D; d++)
            pg[(k * D + d) / W].e[(k * D + d) % W] = gv[d];
    }
}

// the trailing nodes [first, nodes), one at a time (thread 0 of block 0): xv = value(i), g written, done(i, g_i) per unknown
template <class T, class F, class OBJ, class LD, class A, class XV, class DONE>
__device__ __forceinline__ void own_tail(const OBJ& obj, int64_t first, int64_t nodes, T* __restrict__ g, LD ld, A& fx,
                                         XV value, DONE done)
{
    constexpr int D = F::D;
    for (int64_t v = first; v < nodes; v++)
    {
        T xv[D], gv[D];
#pragma unroll
        for (int k = 0; k < D; k++)
            xv[k] = value(v * D + k);
        uint32_t lo, hi;
        if constexpr (OwnRange<F>::value)
            F::range(obj, v, lo, hi);
        else
        {
            const uint32_t* __restrict__ off = F::off(obj);
            lo = off[v];
            hi = off[v + 1];
        }
        F::template node<T>(obj, v, xv, lo, hi, ld, fx, gv);
#pragma unroll
        for (int k = 0; k < D; k++)
        {
            g[v * D + k] = gv[k];
            done(v * D + k, gv[k]);
        }
    }
}

// ---------------------------------------------------------------- k_eval's and k_b_eval's counterparts
// BOUNDED false: out[0] = f(x), out[1] = g.g, out[2] = x.x;  true: out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class F, class OBJ, bool BOUNDED>
__device__ __forceinline__ void own_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                         const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, D = F::D;
    constexpr int NA = BOUNDED ? 2 : 3, XX = NA - 1;  // acc[0]: f's sum, acc[XX]: x.x, acc[1] of three: g.g
    A acc[NA];
    double pgm = 0.0;
    const int64_t nodes = F::nodes(obj, n);
    const int64_t nv = nodes / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    auto ld = [&](int64_t i) { return x[i]; };
    // the tail reads x[i] again instead of carrying it across the node's walk: carried, it costs k_lin_b_eval an occupancy step
    auto done = [&](int64_t i, T gi) __attribute__((always_inline)) {
        acc[XX].add_prod(x[i], x[i]);
        if constexpr (BOUNDED)
            pgm = fmax(pgm, double(projg_term(x[i], gi, lb[i], ub[i])));
        else
            acc[1].add_prod(gi, gi);
    };
    for (int64_t vi = int64_t(blockIdx.x) * kBlock + threadIdx.x; vi < nv; vi += stride)
    {
        Pack<T> px[D], pl[D], pu[D], pg[D];
#pragma unroll
        for (int j = 0; j < D; j++)
        {
            px[j] = ldv(x, vi * D + j);
            if constexpr (BOUNDED)
            {
                pl[j] = ldv(lb, vi * D + j);
                pu[j] = ldv(ub, vi * D + j);
            }
        }
        uint32_t o[own_noff<F, W>];
        own_offsets<F, W>(obj, vi * W, o);
        own_group_nodes<T, F>(obj, vi, px, o, ld, acc[0], pg);
#pragma unroll
        for (int j = 0; j < D; j++)
        {
            stv(g, vi * D + j, pg[j]);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[XX].add_prod(px[j].e[k], px[j].e[k]);
                if constexpr (BOUNDED)
                    pgm = fmax(pgm, double(projg_term(px[j].e[k], pg[j].e[k], pl[j].e[k], pu[j].e[k])));
                else
                    acc[1].add_prod(pg[j].e[k], pg[j].e[k]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        own_tail<T, F>(obj, nv * W, nodes, g, ld, acc[0], ld, done);
    F::template extra<T>(obj, acc[0]);
    if constexpr (BOUNDED)
        ext_publish<false>(pgm, ws, 4);
    if (grid_reduce<NA>(acc, ws))
    {
        double pgmax = 0.0;
        if constexpr (BOUNDED)
            pgmax = ext_collect<false>(ws, 4);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[0].value());
            out[1] = T(acc[1].value());
            out[2] = BOUNDED ? T(pgmax) : T(acc[XX].value());
        }
    }
}

// ---------------------------------------------------------------- k_trial's and k_b_dg_maxstep_trial's counterparts
// x = xp + step*d ; g = grad f(x).  BOUNDED false: out[0] = f(x), out[1] = g.d;
// true: out[0] = g0.d, out[1] = step_max, out[2] = f(x), out[3] = grad(x).d
template <class T, class F, class OBJ, bool BOUNDED>
__device__ __forceinline__ void own_trial(const T* __restrict__ xp, const T* __restrict__ g0, const T* __restrict__ d,
                                          const T* __restrict__ lb, const T* __restrict__ ub, T step, T* __restrict__ x,
                                          T* __restrict__ g, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, D = F::D, U = F::U;
    constexpr int NA = BOUNDED ? 3 : 2;
    A acc[NA];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t nodes = F::nodes(obj, n);
    const int64_t nv = nodes / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    auto ld = [&](int64_t i) { return xp[i] + step * d[i]; };
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        Pack<T> pxp[U][D], pd[U][D], pg0[U][D], plo[U][D], pup[U][D];
        uint32_t o[U][own_noff<F, W>];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
#pragma unroll
                for (int j = 0; j < D; j++)
                {
                    pxp[u][j] = ldv<T>(xp, vi * D + j);
                    pd[u][j] = ldv<T>(d, vi * D + j);
                    if constexpr (BOUNDED)
                    {
                        pg0[u][j] = ldv<T>(g0, vi * D + j);
                        plo[u][j] = ldv<T>(lb, vi * D + j);
                        pup[u][j] = ldv<T>(ub, vi * D + j);
                    }
                }
                own_offsets<F, W>(obj, vi * W, o[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                Pack<T> px[D], pg[D];
#pragma unroll
                for (int j = 0; j < D; j++)
#pragma unroll
                    for (int k = 0; k < W; k++)
                    {
                        px[j].e[k] = pxp[u][j].e[k] + step * pd[u][j].e[k];
                        if constexpr (BOUNDED)
                        {
                            acc[NA - 1].add_prod(pg0[u][j].e[k], pd[u][j].e[k]);
                            feas(pxp[u][j].e[k], pd[u][j].e[k], plo[u][j].e[k], pup[u][j].e[k]);
                        }
                    }
                own_group_nodes<T, F>(obj, vi, px, o[u], ld, acc[0], pg);
#pragma unroll
                for (int j = 0; j < D; j++)
                {
                    stv<T>(x, vi * D + j, px[j]);
                    stv<T>(g, vi * D + j, pg[j]);
#pragma unroll
                    for (int k = 0; k < W; k++)
                        acc[1].add_prod(pg[j].e[k], pd[u][j].e[k]);
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        own_tail<T, F>(
            obj, nv * W, nodes, g, ld, acc[0],
            [&](int64_t i) __attribute__((always_inline)) {
                if constexpr (BOUNDED)
                {
                    acc[NA - 1].add_prod(g0[i], d[i]);
                    feas(xp[i], d[i], lb[i], ub[i]);
                }
                const T xi = xp[i] + step * d[i];
                x[i] = xi;
                return xi;
            },
            [&](int64_t i, T gi) __attribute__((always_inline)) { acc[1].add_prod(gi, d[i]); });
    F::template extra<T>(obj, acc[0]);
    if constexpr (BOUNDED)
        ext_publish<true>(smin, ws, 6);
    if (grid_reduce<NA>(acc, ws))
    {
        double smin_all = 0.0;
        if constexpr (BOUNDED)
            smin_all = ext_collect<true>(ws, 6);
        if (threadIdx.x == 0)
        {
            if constexpr (BOUNDED)
            {
                out[0] = T(acc[2].value());
                out[1] = T(smin_all);
            }
            out[BOUNDED ? 2 : 0] = T(acc[0].value());
            out[BOUNDED ? 3 : 1] = T(acc[1].value());
            ws_signal(ws);
        }
    }
}

// ---------------------------------------------------------------- the four kernels of a family
// PREFIX_eval, PREFIX_trial, PREFIX_b_eval and PREFIX_b_dg_maxstep_trial for the family FAMILY (frame_kernels.cuh)
#define LBFGSX_OWN_KERNELS(PREFIX, FAMILY) LBFGSX_FRAME_KERNELS(PREFIX, own_eval, own_trial, FAMILY)

}  // namespace lbfgsx
