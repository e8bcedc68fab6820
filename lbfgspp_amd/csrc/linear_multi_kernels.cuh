// lbfgspp_amd/csrc/linear_multi_kernels.cuh -- the evaluation kernels for a MULTI-OUTPUT LINEAR-MODEL objective
//     f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r),      Z = A X,
// A sparse, R x F, given in CSR; x holds the F x D weight matrix X feature-major, x[j*D + c], n = F*D; D = OBJ::D is a
// compile-time constant of the generated struct, 1 .. 16 (include/lbfgsx.h, "multi-output linear-model objectives").
//
// It is the scalar form (linear_kernels.cuh) with D values where that has one, and shares its matrix, its launches and its
// argument struct (launch_args.hpp: LinearArgs; linear_topology.hip builds the lists over the F columns):
//   the ROW pass    k_linm_rows / k_linm_rows_trial    Z[r, :], then w[r*D + c] = dphi/dz_c and v[r] = phi
//   the COLUMN pass k_linm_eval, k_linm_trial, k_linm_b_eval, k_linm_b_dg_maxstep_trial: own_eval / own_trial (own_frame.cuh)
//                   with the arguments, grids, tile order, reductions and completion signal of the scalar form's four.
// OBJ is the struct generated around the caller's two texts,
//     static constexpr int D;  static constexpr bool kCoord;   T coord(const T (&x)[1], T (&g)[1], int64_t i) const;
//     T row(const T (&z)[D], T (&dz)[D], int64_t r) const;      and the members of LinearArgs.
//
// Row sums.  Z[r, c] is the scalar form's row sum for each c on its own: L lanes share a row, lane l takes the entries
// k0+l, k0+l+L, .. in ascending order, s_l[c] = val[k]*x[col[k]*D + c] for its first entry and s_l[c] = s_l[c] + .. after it,
// +0 without one; then s_l[c] = s_l[c] + s_{l+h}[c] for l < h, h = L/2 .. 1, by D cross-lane moves per halving: no LDS, no
// atomic.  A lane reads the D contiguous values of a feature's weight row, with 16-byte loads when D*sizeof(T) is a multiple
// of 16 (every row of X is then aligned).  linm_group<T, D>() entries are in flight together: as many as keep the gathered
// values of the trial form (xp and d) within 256 bytes per lane, so D = 16 in f64 does not spill.  Lane 0 runs the row body.
//
// Gradient.  A thread owns one 16-byte pack of consecutive COORDINATES, the frame's D = 1 ownership (not W features x D
// packs: at D = 10 that is over 200 registers in the bounded trial kernel).  Coordinate i = j*D + c walks the list of
// feature j: psi's g[0] if there is a coordinate body, then tval[q]*w[trow[q]*D + c] over q in [colptr[j], colptr[j+1]) in
// ascending q from the first contribution, +0 without any.  colptr has F + 1 entries, so the family supplies (lo, hi) per
// coordinate (own_frame.cuh: kRange); a pack may straddle two features when D is odd.  A feature's D coordinates read the
// same entries: the re-reads are cache hits.  A long column (more than C entries) has D partials per chunk, part[b*D + c],
// written by k_lin_long_cols_multi (linear_topology.hip) and added by the owner in ascending b.
//
// f.  As the scalar form: psi's values by the owners, and every row's value from v[R] by the same launch.
//
// Every index read here was validated at bind: 0 <= col < F, 0 <= trow < R, list positions in [0, nnz).
#pragma once
#include "linear_kernels.cuh"

namespace lbfgsx {

// entries whose loads are in flight together in the row pass
template <class T, int D>
__host__ __device__ constexpr int linm_group()
{
    return (2 * D * int(sizeof(T)) <= 64) ? 4 : (2 * D * int(sizeof(T)) <= 128) ? 2 : 1;
}

// ---------------------------------------------------------------- the row pass
// the D values at p[0..D): 16-byte loads where every weight row is aligned
template <class T, int D>
__device__ __forceinline__ void linm_load(const T* __restrict__ p, T (&out)[D])
{
    constexpr int W = Vec16<T>::W;
    if constexpr ((D * int(sizeof(T))) % 16 == 0)
    {
#pragma unroll
        for (int j = 0; j < D / W; j++)
        {
            const Pack<T> pk = ldv(p, j);
#pragma unroll
            for (int k = 0; k < W; k++)
                out[j * W + k] = pk.e[k];
        }
    }
    else
    {
#pragma unroll
        for (int c = 0; c < D; c++)
            out[c] = p[c];
    }
}

// ld(j, xj) fills xj[0..D) with the weight row of feature j -- from memory in k_linm_rows, recomputed from xp and d in
// k_linm_rows_trial
template <class T, class OBJ, class LD>
__device__ __forceinline__ void linm_rows(const OBJ& obj, LD ld)
{
    constexpr int D = OBJ::D, G = linm_group<T, D>();
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
        T s[D];
#pragma unroll
        for (int c = 0; c < D; c++)
            s[c] = T(0);
        bool has = false;
        for (; k < k1; k += int64_t(G) * L)
        {
            int32_t cj[G];
            T vj[G], xj[G][D];
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
                if (k + int64_t(j) * L < k1)
                    ld(int64_t(cj[j]), xj[j]);
#pragma unroll
            for (int j = 0; j < G; j++)
                if (k + int64_t(j) * L < k1)
                {
#pragma unroll
                    for (int c = 0; c < D; c++)
                    {
                        const T prod = vj[j] * xj[j][c];
                        s[c] = has ? s[c] + prod : prod;
                    }
                    has = true;
                }
        }
        // lanes l >= h compute values nobody reads; all lanes of the wavefront take part in every move
        for (int h = L >> 1; h >= 1; h >>= 1)
        {
#pragma unroll
            for (int c = 0; c < D; c++)
                s[c] = s[c] + __shfl_down(s[c], unsigned(h), L);
        }
        if (live && lane == 0)
        {
            T dz[D];
#pragma unroll
            for (int c = 0; c < D; c++)
                dz[c] = T(0);
            const T value = obj.row(s, dz, r);
#pragma unroll
            for (int c = 0; c < D; c++)
                obj.w[r * D + c] = dz[c];
            obj.v[r] = value;
        }
    }
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_rows(const T* __restrict__ x, OBJ obj)
{
    constexpr int D = OBJ::D;
    linm_rows<T>(obj, [&](int64_t j, T(&xj)[D]) __attribute__((always_inline)) { linm_load<T, D>(x + j * D, xj); });
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    constexpr int D = OBJ::D;
    linm_rows<T>(obj, [&](int64_t j, T(&xj)[D]) __attribute__((always_inline)) {
        T a[D], b[D];
        linm_load<T, D>(xp + j * D, a);
        linm_load<T, D>(d + j * D, b);
#pragma unroll
        for (int c = 0; c < D; c++)
            xj[c] = a[c] + step * b[c];
    });
}

// ---------------------------------------------------------------- the column pass
// coordinate i = j*D + c with value xi and feature j's transposed entries [lo, hi): its gradient, returned; psi's value
// goes to fx.  lin_coord (linear_kernels.cuh) with w[r*D + c] for w[r] and part[q*D + c] for part[q]
template <class T, class OBJ, class A>
__device__ __forceinline__ T linm_coord(const OBJ& obj, int64_t i, T xi, uint32_t lo, uint32_t hi, A& fx)
{
    constexpr int G = kLinGroup, D = OBJ::D;
    const int64_t j = i / D;
    const int c = int(i - j * D);
    T gv = T(0);
    bool has = false;
    if (OBJ::kCoord)
    {
        const T tx[1] = {xi};
        T tg[1];
        fx.add(obj.coord(tx, tg, i));
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
            const T pq = part[int64_t(q) * D + c];
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
                wj[t] = w[int64_t(rj[t]) * D + c];
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

// the frame's family (own_frame.cuh): n coordinates, each with the list of its feature (kRange: colptr has F + 1 entries,
// not n + 1), and every row's value as the extra pass
struct LinMultiFamily
{
    static constexpr int D = 1, U = kLinTrialU;
    static constexpr bool kRange = true;
    template <class OBJ>
    static __device__ __forceinline__ int64_t nodes(const OBJ&, int64_t n)
    {
        return n;
    }
    template <class OBJ>
    static __device__ __forceinline__ void range(const OBJ& obj, int64_t i, uint32_t& lo, uint32_t& hi)
    {
        const uint32_t* __restrict__ colptr = obj.colptr;
        const int64_t j = i / OBJ::D;
        lo = colptr[j];
        hi = colptr[j + 1];
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t i, const T (&xi)[1], uint32_t lo, uint32_t hi, LD, A& fx,
                                                T (&gi)[1])
    {
        gi[0] = linm_coord<T>(obj, i, xi[0], lo, hi, fx);
    }
    template <class T, class OBJ, class A>
    static __device__ __forceinline__ void extra(const OBJ& obj, A& fx)
    {
        lin_row_values<T>(obj, fx);
    }
};

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                      T* __restrict__ out)
{
    own_eval<T, LinMultiFamily, OBJ, false>(x, g, nullptr, nullptr, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                        const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                        T* __restrict__ out)
{
    own_eval<T, LinMultiFamily, OBJ, true>(x, g, lb, ub, n, obj, ws, out);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                       T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out, int rev)
{
    own_trial<T, LinMultiFamily, OBJ, false>(xp, nullptr, d, nullptr, nullptr, step, x, g, n, obj, ws, out, rev);
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_linm_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                    const T* __restrict__ d, const T* __restrict__ lb,
                                                                    const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                    T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                    T* __restrict__ out, int rev)
{
    own_trial<T, LinMultiFamily, OBJ, true>(xp, g0, d, lb, ub, step, x, g, n, obj, ws, out, rev);
}

}  // namespace lbfgsx
