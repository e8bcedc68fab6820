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
#include "own_frame.cuh"
#include "graph_entry.hpp"

namespace lbfgsx {

constexpr int kGraphGroup = 4;   // entries whose loads are in flight together
constexpr int kGraphTrialU = 2;  // the tile depth of the two trial kernels

// the walk of node v with value xv over its entries [lo, hi): g_e[side] of each added to gv, which holds what precedes them in
// the node's sum; the values of the edges v is end 0 of go to fx.  ld(u) = x[u] -- from memory in the evaluation kernels,
// recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ void graph_walk(const OBJ& obj, int64_t v, T xv, uint32_t lo, uint32_t hi, LD ld, A& fx, LinSum<T>& gv)
{
    constexpr int G = kGraphGroup;
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
                gv.add(far ? tg[1] : tg[0]);
                if (!far)
                    fx.add(val);
            }
    }
}

// node v with value xv and entries [lo, hi): its gradient, returned; its node value and the values of the edges it is end 0
// of go to fx
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T graph_node(const OBJ& obj, int64_t v, T xv, uint32_t lo, uint32_t hi, LD ld, A& fx)
{
    LinSum<T> gv;
    if (OBJ::kNode)
    {
        const T tx[1] = {xv};
        T tg[1];
        fx.add(obj.node(tx, tg, v));
        gv.add(tg[0]);
    }
    graph_walk<T>(obj, v, xv, lo, hi, ld, fx, gv);
    return gv.value;
}

// the frame's family (own_frame.cuh): n nodes of one unknown, the list at off, no extra pass
struct GraphFamily
{
    static constexpr int D = 1, U = kGraphTrialU;
    template <class OBJ>
    static __device__ __forceinline__ int64_t nodes(const OBJ&, int64_t n)
    {
        return n;
    }
    template <class OBJ>
    static __device__ __forceinline__ const uint32_t* off(const OBJ& obj)
    {
        return obj.off;
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t v, const T (&xv)[1], uint32_t lo, uint32_t hi, LD ld,
                                                A& fx, T (&gv)[1])
    {
        gv[0] = graph_node<T>(obj, v, xv[0], lo, hi, ld, fx);
    }
    template <class T, class OBJ, class A>
    static __device__ __forceinline__ void extra(const OBJ&, A&)
    {
    }
};

// k_graph_eval, k_graph_trial, k_graph_b_eval, k_graph_b_dg_maxstep_trial
LBFGSX_OWN_KERNELS(k_graph, GraphFamily)

}  // namespace lbfgsx
