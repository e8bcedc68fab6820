// lbfgspp_amd/csrc/mesh_kernels.cuh -- the four evaluation kernels for a MESH objective
//     f(x) = sum over nodes v of psi(x_v; v)  +  sum over elements e of phi(x at the K nodes of e; e),
// N nodes of D unknowns each, x node-major (x[v*D + d], n = N*D), E elements of K nodes (include/lbfgsx.h, "mesh objectives").
//
// k_mesh_eval, k_mesh_trial, k_mesh_b_eval and k_mesh_b_dg_maxstep_trial take the arguments of their k_graph_* counterparts
// (graph_kernels.cuh) and are launched with their grids: the same outputs, tile order, reductions and completion signal.
// Compiled at run time only (jit_objective.hip); OBJ is the struct generated around the caller's two texts,
//     static constexpr int K, D;  static constexpr bool kNode;
//     T node(const T (&x)[D], T (&g)[D], int64_t i) const;
//     T elem(const T (&x)[K*D], T (&g)[K*D], int64_t e, const int64_t (&v)[K]) const;
//     const uint32_t* off; const uint32_t* inc; int64_t E, N;
//
// The list (mesh_topology.hip, from validated indices): node v's entries are off[v] .. off[v+1], in ascending e; an entry is
// K 32-bit words: (e << 2) | slot -- v is node `slot` of element e -- then the element's other nodes in ascending slot order.
//
// Ownership.  A thread owns W = 16 / sizeof(T) consecutive nodes: exactly D whole 16-byte packs of x from pack vi*D; thread
// 0 of block 0 also owns the N mod W trailing nodes.  The owner of v writes grad[v*D .. v*D+D): psi's g if there is a node
// term, then g_e[slot*D + d] of v's entries in list order, started from the first contribution; +0 if there is none.  It adds
// psi's value to f, and an element's value when v is its slot 0.  An element is thus evaluated K times on identical inputs
// by the same instructions: the same bits, no float atomic.
//
// The walk.  Groups of mesh_group<T, K, D>() entries: the group's entry loads before its gathers, the gathers before its
// terms.  The own slot is a run-time value: the body's inputs and the partials kept are picked with unrolled
// compare-and-select, never with a run-time index into a register array; one inlined copy of the body serves all slots.  In
// the trial kernels a gathered value is xp[u] + step*d[u], never a read of the x this launch writes.  Every index read from
// the list was validated at bind, every list position lies in [0, K*E).
#pragma once
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"

namespace lbfgsx {

// the tile depth of the two trial kernels: the dg / max-step kernel holds five vectors of D packs per tile row
template <int D>
struct MeshTrialU
{
    static constexpr int value = (D == 1) ? 2 : 1;
};

// entries whose loads are in flight together, by the 32-bit registers one entry's gathered values take
template <class T, int K, int D>
__host__ __device__ constexpr int mesh_group()
{
    return ((K - 1) * D * int(sizeof(T)) <= 16) ? 4 : ((K - 1) * D * int(sizeof(T)) <= 32) ? 2 : 1;
}

// one entry: K words, loaded with one instruction where the alignment allows it
template <int K>
struct alignas(K == 3 ? 4 : 4 * K) MeshEntry
{
    uint32_t w[K];
};

// the W + 1 offsets of the node group at b = vi*W (off has N + 1 elements, b + W <= N)
template <int W>
__device__ __forceinline__ void mesh_offsets(const uint32_t* __restrict__ off, int64_t b, uint32_t (&o)[W + 1])
{
#pragma unroll
    for (int k = 0; k <= W; k++)
        o[k] = off[b + k];
}

// node v with values xv and entries [lo, hi): its D partial derivatives go to gv; its node value and the values of the
// elements it is slot 0 of go to fx.  ld(i) = x[i] -- from memory in the evaluation kernels, recomputed from xp and d in
// the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ void mesh_node(const OBJ& obj, int64_t v, const T (&xv)[OBJ::D], uint32_t lo, uint32_t hi, LD ld,
                                          A& fx, T (&gv)[OBJ::D])
{
    constexpr int K = OBJ::K, D = OBJ::D;
    constexpr int G = mesh_group<T, K, D>();
    bool has = false;
#pragma unroll
    for (int d = 0; d < D; d++)
        gv[d] = T(0);
    if (OBJ::kNode)
    {
        fx.add(obj.node(xv, gv, v));
        has = true;
    }
    const MeshEntry<K>* __restrict__ inc = reinterpret_cast<const MeshEntry<K>*>(obj.inc);
    for (int64_t q = lo; q < int64_t(hi); q += G)
    {
        MeshEntry<K> en[G];
        T xo[G][(K - 1) * D];
#pragma unroll
        for (int j = 0; j < G; j++)
        {
#pragma unroll
            for (int k = 0; k < K; k++)
                en[j].w[k] = 0;
            if (q + j < int64_t(hi))
                en[j] = inc[q + j];
        }
#pragma unroll
        for (int j = 0; j < G; j++)
        {
#pragma unroll
            for (int k = 0; k < (K - 1) * D; k++)
                xo[j][k] = T(0);
            if (q + j < int64_t(hi))
            {
#pragma unroll
                for (int k = 0; k < K - 1; k++)
#pragma unroll
                    for (int d = 0; d < D; d++)
                        xo[j][k * D + d] = ld(int64_t(en[j].w[k + 1]) * D + d);
            }
        }
#pragma unroll
        for (int j = 0; j < G; j++)
            if (q + j < int64_t(hi))
            {
                const int slot = int(en[j].w[0] & 3u);
                T tx[K * D], tg[K * D];
                int64_t tv[K];
                // slot k of the element is v itself (k == slot), the k-th other node (k < slot) or the (k-1)-th (k > slot)
#pragma unroll
                for (int k = 0; k < K; k++)
                {
                    const int lo_k = (k < K - 1) ? k : K - 2;  // the other node taken when k < slot
                    const int hi_k = (k > 0) ? k - 1 : 0;      // and when k > slot
                    tv[k] = (k == slot) ? v : int64_t(k < slot ? en[j].w[1 + lo_k] : en[j].w[1 + hi_k]);
#pragma unroll
                    for (int d = 0; d < D; d++)
                        tx[k * D + d] = (k == slot) ? xv[d] : (k < slot ? xo[j][lo_k * D + d] : xo[j][hi_k * D + d]);
                }
                const T val = obj.elem(tx, tg, int64_t(en[j].w[0] >> 2), tv);
#pragma unroll
                for (int d = 0; d < D; d++)
                {
                    T mine = tg[d];
#pragma unroll
                    for (int k = 1; k < K; k++)
                        mine = (slot == k) ? tg[k * D + d] : mine;
                    gv[d] = has ? gv[d] + mine : mine;
                }
                has = true;
                if (slot == 0)
                    fx.add(val);
            }
    }
}

// the W nodes of group vi: their values from the D packs px, their gradients into the D packs pg
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ void mesh_group_nodes(const OBJ& obj, int64_t vi, const Pack<T> (&px)[OBJ::D],
                                                 const uint32_t (&o)[Vec16<T>::W + 1], LD ld, A& fx, Pack<T> (&pg)[OBJ::D])
{
    constexpr int W = Vec16<T>::W, D = OBJ::D;
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        T xv[D], gv[D];
#pragma unroll
        for (int d = 0; d < D; d++)
            xv[d] = px[(k * D + d) / W].e[(k * D + d) % W];
        mesh_node<T>(obj, vi * W + k, xv, o[k], o[k + 1], ld, fx, gv);
#pragma unroll
        for (int d = 0; d < D; d++)
            pg[(k * D + d) / W].e[(k * D + d) % W] = gv[d];
    }
}

// the N mod W trailing nodes, one at a time (thread 0 of block 0): xv = value(i), g written, done(i, g_i) per unknown
template <class T, class OBJ, class LD, class A, class XV, class DONE>
__device__ __forceinline__ void mesh_tail(const OBJ& obj, int64_t first, T* __restrict__ g, LD ld, A& fx, XV value, DONE done)
{
    constexpr int D = OBJ::D;
    for (int64_t v = first; v < obj.N; v++)
    {
        T xv[D], gv[D];
#pragma unroll
        for (int k = 0; k < D; k++)
            xv[k] = value(v * D + k);
        mesh_node<T>(obj, v, xv, obj.off[v], obj.off[v + 1], ld, fx, gv);
#pragma unroll
        for (int k = 0; k < D; k++)
        {
            g[v * D + k] = gv[k];
            done(v * D + k, xv[k], gv[k]);
        }
    }
}

// ---------------------------------------------------------------- k_graph_eval's and k_graph_b_eval's counterparts
// BOUNDED false: out[0] = f(x), out[1] = g.g, out[2] = x.x;  true: out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class OBJ, bool BOUNDED>
__device__ __forceinline__ void mesh_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                          const T* __restrict__ ub, OBJ obj, RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, D = OBJ::D;
    constexpr int NA = BOUNDED ? 2 : 3, XX = NA - 1;  // acc[0]: f's sum, acc[XX]: x.x, acc[1] of three: g.g
    A acc[NA];
    double pgm = 0.0;
    const int64_t nv = obj.N / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    auto ld = [&](int64_t i) { return x[i]; };
    auto done = [&](int64_t i, T xi, T gi) __attribute__((always_inline)) {
        acc[XX].add_prod(xi, xi);
        if constexpr (BOUNDED)
            pgm = fmax(pgm, double(projg_term(xi, gi, lb[i], ub[i])));
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
        uint32_t o[W + 1];
        mesh_offsets<W>(obj.off, vi * W, o);
        mesh_group_nodes<T>(obj, vi, px, o, ld, acc[0], pg);
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
        mesh_tail<T>(obj, nv * W, g, ld, acc[0], ld, done);
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

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_mesh_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                      T* __restrict__ out)
{
    mesh_eval<T, OBJ, false>(x, g, nullptr, nullptr, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_mesh_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                        const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                        T* __restrict__ out)
{
    mesh_eval<T, OBJ, true>(x, g, lb, ub, obj, ws, out);
}

// ---------------------------------------------------------------- k_graph_trial's and k_graph_b_dg_maxstep_trial's counterparts
// x = xp + step*d ; g = grad f(x).  BOUNDED false: out[0] = f(x), out[1] = g.d;
// true: out[0] = g0.d, out[1] = step_max, out[2] = f(x), out[3] = grad(x).d
template <class T, class OBJ, bool BOUNDED>
__device__ __forceinline__ void mesh_trial(const T* __restrict__ xp, const T* __restrict__ g0, const T* __restrict__ d,
                                           const T* __restrict__ lb, const T* __restrict__ ub, T step, T* __restrict__ x,
                                           T* __restrict__ g, OBJ obj, RedWs ws, T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, D = OBJ::D;
    constexpr int U = MeshTrialU<D>::value;
    constexpr int NA = BOUNDED ? 3 : 2;
    A acc[NA];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t nv = obj.N / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    auto ld = [&](int64_t i) { return xp[i] + step * d[i]; };
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        Pack<T> pxp[U][D], pd[U][D], pg0[U][D], plo[U][D], pup[U][D];
        uint32_t o[U][W + 1];
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
                mesh_offsets<W>(obj.off, vi * W, o[u]);
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
                mesh_group_nodes<T>(obj, vi, px, o[u], ld, acc[0], pg);
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
        mesh_tail<T>(
            obj, nv * W, g, ld, acc[0],
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
            [&](int64_t i, T, T gi) __attribute__((always_inline)) { acc[1].add_prod(gi, d[i]); });
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

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_mesh_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                       T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out, int rev)
{
    mesh_trial<T, OBJ, false>(xp, nullptr, d, nullptr, nullptr, step, x, g, obj, ws, out, rev);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_mesh_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                    const T* __restrict__ d, const T* __restrict__ lb,
                                                                    const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                    T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                    T* __restrict__ out, int rev)
{
    mesh_trial<T, OBJ, true>(xp, g0, d, lb, ub, step, x, g, obj, ws, out, rev);
}

}  // namespace lbfgsx
