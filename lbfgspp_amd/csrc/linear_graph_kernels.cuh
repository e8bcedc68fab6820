// lbfgspp_amd/csrc/linear_graph_kernels.cuh -- the evaluation kernels for a GRAPH-REGULARISED LINEAR-MODEL objective
//     f(x) = sum over coordinates j of psi(x[j]; j)  +  sum over edges e of rho(x[ei[e]], x[ej[e]]; e)
//            +  sum over rows r of phi(z_r; r),      z = A x,
// A sparse, R x n, in CSR and E edges over the n coordinates as an index list (include/lbfgsx.h, "graph-regularised
// linear-model objectives"): the scalar linear-model form of linear_kernels.cuh with the edge term of graph_kernels.cuh in its
// column pass.
//
// An evaluation is the linear-model form's: the row pass (k_lin_rows / k_lin_rows_trial, instantiated for this form's struct),
// the long-column launch when the matrix has a long column (k_lin_long_cols, linear_topology.hip), then the column pass
// k_ling_eval, k_ling_trial, k_ling_b_eval, k_ling_b_dg_maxstep_trial, which take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial.  They are compiled at run time only (jit_objective.hip): OBJ is the struct generated around the
// caller's three texts,
//     static constexpr bool kCoord;           T coord(const T (&x)[1], T (&g)[1], int64_t i) const;
//     T edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j) const;
//     T row(T z, T& dz, int64_t r) const;     the members of LinearArgs, then off, inc and E (launch_args.hpp: LinearGraphArgs).
//
// The owner of coordinate j writes grad[j]: psi's g[0] if there is a coordinate body (lin_coord's start), then g_e[side] of j's
// incidence entries in ascending e (graph_walk: an edge is evaluated from both ends on identical inputs), then the column's
// contributions as lin_coord forms them -- tval[q]*w[trow[q]] in ascending q, or a long column's chunk partials in ascending
// chunk index --, all into one sum that starts from its first contribution; +0 if there is none.  It is lin_coord itself with
// graph_walk as what comes between psi's term and the column (lin_coord's mid): neither walk is written twice.  It adds psi's
// value and the values of the edges it is end 0 of to f's accumulator; the launch adds every row's value (lin_row_values).  In
// the trial kernels a gathered other end is xp[u] + step*d[u], as a gathered x[col] is in the row pass: never a read of the x
// the launch writes.  One pass streams x, xp, d, g, lb and ub once for both terms.
//
// The frame hands a node the range of its column (colptr is the frame's offsets); the node loads its two graph offsets itself,
// next to the walk that uses them, so that nothing of the graph list is carried across the tile's loads.  No LDS, no float
// atomic.  Every index read here was validated at bind (graph_topology.hip, linear_topology.hip).
#pragma once
#include "graph_kernels.cuh"
#include "linear_kernels.cuh"

namespace lbfgsx {

struct LinGraphFamily : LinFamilyBase
{
    template <class OBJ>
    static __device__ __forceinline__ const uint32_t* off(const OBJ& obj)
    {
        return obj.colptr;
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t i, const T (&xi)[1], uint32_t lo, uint32_t hi, LD ld,
                                                A& fx, T (&gi)[1])
    {
        // lin_coord's sum with the node's edges between psi's term and the column's contributions
        gi[0] = lin_coord<T>(obj, i, xi[0], lo, hi, fx, [&](LinSum<T>& gv) __attribute__((always_inline)) {
            const uint32_t* __restrict__ off = obj.off;
            const uint32_t elo = off[i], ehi = off[i + 1];
            graph_walk<T>(obj, i, xi[0], elo, ehi, ld, fx, gv);
        });
    }
};

// k_ling_eval, k_ling_trial, k_ling_b_eval, k_ling_b_dg_maxstep_trial
LBFGSX_OWN_KERNELS(k_ling, LinGraphFamily)

}  // namespace lbfgsx
