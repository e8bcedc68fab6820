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
#include "own_frame.cuh"

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

// the frame's family (own_frame.cuh): N nodes of D unknowns, the list at off, no extra pass
template <class OBJ>
struct MeshFamily
{
    static constexpr int D = OBJ::D, U = MeshTrialU<D>::value;
    static __device__ __forceinline__ int64_t nodes(const OBJ& obj, int64_t) { return obj.N; }
    static __device__ __forceinline__ const uint32_t* off(const OBJ& obj) { return obj.off; }
    template <class T, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t v, const T (&xv)[D], uint32_t lo, uint32_t hi, LD ld,
                                                A& fx, T (&gv)[D])
    {
        mesh_node<T>(obj, v, xv, lo, hi, ld, fx, gv);
    }
    template <class T, class A>
    static __device__ __forceinline__ void extra(const OBJ&, A&)
    {
    }
};

// k_mesh_eval, k_mesh_trial, k_mesh_b_eval, k_mesh_b_dg_maxstep_trial (OBJ is the kernels' own template parameter)
LBFGSX_OWN_KERNELS(k_mesh, MeshFamily<OBJ>)

}  // namespace lbfgsx
