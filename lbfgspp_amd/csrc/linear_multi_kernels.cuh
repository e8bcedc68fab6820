// lbfgspp_amd/csrc/linear_multi_kernels.cuh -- the evaluation kernels for a MULTI-OUTPUT LINEAR-MODEL objective
//     f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r),      Z = A X,
// A sparse, R x F, given in CSR; x holds the F x D weight matrix X feature-major, x[j*D + c], n = F*D; D = OBJ::D is a
// compile-time constant of the generated struct, 1 .. 16 (include/lbfgsx.h, "multi-output linear-model objectives").
//
// It is the scalar form (linear_kernels.cuh) with D values where that has one: the same row pass (lin_rows) and column walk
// (lin_coord), which take D from the struct, the same matrix, launches and argument struct (launch_args.hpp: LinearArgs;
// linear_topology.hip builds the lists over the F columns):
//   the ROW pass    k_linm_rows / k_linm_rows_trial    Z[r, :], then w[r*D + c] = dphi/dz_c and v[r] = phi
//   the COLUMN pass k_linm_eval, k_linm_trial, k_linm_b_eval, k_linm_b_dg_maxstep_trial: own_eval / own_trial (own_frame.cuh)
//                   with the arguments, grids, tile order, reductions and completion signal of the scalar form's four.
// OBJ is the struct generated around the caller's two texts,
//     static constexpr int D;  static constexpr bool kCoord;   T coord(const T (&x)[1], T (&g)[1], int64_t i) const;
//     T row(const T (&z)[D], T (&dz)[D], int64_t r) const;      and the members of LinearArgs.
//
// Gradient.  A thread owns one 16-byte pack of consecutive COORDINATES, the frame's D = 1 ownership (not W features x D
// packs: at D = 10 that is over 200 registers in the bounded trial kernel).  Coordinate i = j*D + c walks the list of
// feature j.  colptr has F + 1 entries, so the family supplies (lo, hi) per coordinate (LinFamily<true>; own_frame.cuh:
// kRange); a pack may straddle two features when D is odd.  A feature's D coordinates read the same entries: the re-reads are
// cache hits.  A long column (more than C entries) has D partials per chunk, part[b*D + c], written by k_lin_long_cols
// (linear_topology.hip) with one block per (chunk, output).
//
// With D = 1 every statement here is the scalar form's, and so are the bits.
#pragma once
#include "linear_kernels.cuh"

namespace lbfgsx {

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_rows(const T* __restrict__ x, OBJ obj)
{
    lin_rows<T, LinCsr<T>>(obj, LinGather<T, OBJ::D>{x});
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    lin_rows<T, LinCsr<T>>(obj, LinGatherTrial<T, OBJ::D>{xp, d, step});
}

// k_linm_eval, k_linm_trial, k_linm_b_eval, k_linm_b_dg_maxstep_trial
LBFGSX_OWN_KERNELS(k_linm, LinFamily<true>)

}  // namespace lbfgsx
