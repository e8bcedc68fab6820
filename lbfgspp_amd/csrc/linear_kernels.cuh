// lbfgspp_amd/csrc/linear_kernels.cuh -- the evaluation kernels for a LINEAR-MODEL objective
//     f(x) = sum over coordinates j of psi(x[j]; j)  +  sum over rows r of phi(z_r; r),      z = A x,
// A sparse, R x n, given in CSR (include/lbfgsx.h, "linear-model objectives"), and the row pass and the column walk that the
// multi-output and the dense form (linear_multi_kernels.cuh, linear_dense_kernels.cuh) share with it: a row has D outputs,
// D = OBJ::D where the generated struct has that member and 1 for the struct of this form, which has none (lin_outputs).
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
// Row sums (lin_rows, the one row pass of the three forms).  x holds D values per column c of the matrix, x[c*D ..].  L lanes
// share one row (L a power of two <= 64, fixed at bind, so a group never leaves its wavefront).  Lane l takes the row's
// entries k0+l, k0+l+L, .. in ascending order, s_l[o] = val[k]*x[col[k]*D + o] for its first entry and s_l[o] = s_l[o] + ..
// after it; a lane with no entry holds +0.  Then s_l[o] = s_l[o] + s_{l+h}[o] for l < h, h = L/2 .. 1, by D cross-lane moves
// per halving inside the group: no LDS allocation, no atomic, no reduction workspace.  z_r = s_0, and lane 0 runs the row body.
// A block handles kBlock / L rows per step and strides over the grid.  Where a row's entries come from is the pass's SRC: CSR
// here (LinCsr), the dense row in linear_dense_kernels.cuh.  A lane reads the D contiguous values of a column with 16-byte
// loads when D*sizeof(T) is a multiple of 16 (every such group is then aligned).  linm_group<T, D>() entries are in flight
// together: as many as keep the gathered values of the trial form (xp and d) within 256 bytes per lane, so D = 16 in f64 does
// not spill; 4 at D = 1.  In the trial form the gathered value is xp[i] + step*d[i], the statement i's owner executes in the
// column pass that follows: never a read of the x that pass writes.
//
// Gradient (lin_coord, the one column walk of the two sparse forms).  A thread owns the W coordinates of a 16-byte pack;
// thread 0 of block 0 also owns the coordinates past the last whole pack.  The owner of coordinate i = j*D + o writes grad[i]:
// psi's g[0] if there is a coordinate body, then tval[q]*w[trow[q]*D + o] over the entries q in [colptr[j], colptr[j+1]) of
// the transposed list (ascending r, the caller's order within one r), started from the first contribution (no leading 0 +);
// +0 if there is none.  A column with more than C entries is LONG: its chunk partials part[b*D + o] were written by
// k_lin_long_cols (linear_topology.hip) and the owner adds them in ascending chunk index b instead of walking the entries.
// Entry loads are issued in groups of kLinGroup ahead of the w gathers, the gathers ahead of the arithmetic.
//
// f.  The owner adds psi's value; the same launch strides over v[R] in packs and adds every row's value to the same
// order-independent accumulator (reduce.cuh).
//
// Every index read here was validated at bind: 0 <= col < n / D, 0 <= trow < R, list positions in [0, nnz).
#pragma once
#include "own_frame.cuh"

namespace lbfgsx {

constexpr int kLinGroup = 4;   // entries whose loads are in flight together in the column walk
constexpr int kLinTrialU = 2;  // the tile depth of the two trial column kernels

// the outputs of a row: OBJ::D, or 1 for a struct without that member, whose row body takes scalars
template <class OBJ, class = void>
struct LinOutputs
{
    static constexpr int value = 1;
    static constexpr bool kScalarRow = true;
};
template <class OBJ>
struct LinOutputs<OBJ, decltype(void(OBJ::D))>
{
    static constexpr int value = OBJ::D;
    static constexpr bool kScalarRow = false;
};
template <class OBJ>
constexpr int lin_outputs = LinOutputs<OBJ>::value;

// entries whose loads are in flight together in the row pass
template <class T, int D>
__host__ __device__ constexpr int linm_group()
{
    return (2 * D * int(sizeof(T)) <= 64) ? 4 : (2 * D * int(sizeof(T)) <= 128) ? 2 : 1;
}

// ---------------------------------------------------------------- the row pass
// the D values at p[0..D): 16-byte loads where every group of D is aligned
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

// what the row pass gathers for column j, ld(j, xj): the D values x[j*D ..] from memory ..
template <class T, int D>
struct LinGather
{
    const T* __restrict__ x;
    __device__ __forceinline__ void operator()(int64_t j, T (&xj)[D]) const { linm_load<T, D>(x + j * D, xj); }
};
// .. and recomputed from xp and d in the trial form
template <class T, int D>
struct LinGatherTrial
{
    const T* __restrict__ xp;
    const T* __restrict__ d;
    T step;
    __device__ __forceinline__ void operator()(int64_t j, T (&xj)[D]) const
    {
        T a[D], b[D];
        linm_load<T, D>(xp + j * D, a);
        linm_load<T, D>(d + j * D, b);
#pragma unroll
        for (int c = 0; c < D; c++)
            xj[c] = a[c] + step * b[c];
    }
};

// the entry source of a CSR matrix.  span: lane `lane` of row r starts at entry k and the row ends before k1, both 0 for a
// row that is not `live` (r >= R).  entry: entry k of that row is (c, v) if it is `in` the row, and (0, +0) if not.  Nothing is
// read for a row that is not live or an entry that is not in
template <class T>
struct LinCsr
{
    typedef int32_t col_t;
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ col;
    const T* __restrict__ val;
    template <class OBJ>
    __device__ __forceinline__ explicit LinCsr(const OBJ& obj) : rowptr(obj.rowptr), col(obj.col), val(obj.val)
    {
    }
    __device__ __forceinline__ void span(int64_t r, bool live, int lane, int64_t& k, int64_t& k1)
    {
        k = k1 = 0;
        if (live)
        {
            k = int64_t(rowptr[r]) + lane;
            k1 = rowptr[r + 1];
        }
    }
    __device__ __forceinline__ void entry(int64_t k, bool in, col_t& c, T& v) const
    {
        c = 0;
        v = T(0);
        if (in)
        {
            c = col[k];
            v = val[k];
        }
    }
};

// the row body on arrays, whichever signature the generated struct has
template <class T, class OBJ, int D>
__device__ __forceinline__ T lin_row_body(const OBJ& obj, const T (&z)[D], T (&dz)[D], int64_t r)
{
    if constexpr (LinOutputs<OBJ>::kScalarRow)
        return obj.row(z[0], dz[0], r);
    else
        return obj.row(z, dz, r);
}

// every row's D sums, its body, w and v.  SRC: where a row's entries come from; ld(j, xj) fills xj[0..D) with the D values
// of column j (LinGather, LinGatherTrial)
template <class T, class SRC, class OBJ, class LD>
__device__ __forceinline__ void lin_rows(const OBJ& obj, LD ld)
{
    constexpr int D = lin_outputs<OBJ>, G = linm_group<T, D>();
    const int L = obj.L;
    const int rpb = kBlock / L;
    const int lane = int(threadIdx.x) & (L - 1);
    const int slot = int(threadIdx.x) / L;
    SRC src(obj);
    for (int64_t r0 = int64_t(blockIdx.x) * rpb; r0 < obj.R; r0 += int64_t(gridDim.x) * rpb)
    {
        const int64_t r = r0 + slot;
        const bool live = r < obj.R;
        int64_t k, k1;
        src.span(r, live, lane, k, k1);
        T s[D];
#pragma unroll
        for (int c = 0; c < D; c++)
            s[c] = T(0);
        bool has = false;
        for (; k < k1; k += int64_t(G) * L)
        {
            typename SRC::col_t cj[G];
            T vj[G], xj[G][D];
#pragma unroll
            for (int j = 0; j < G; j++)
                src.entry(k + int64_t(j) * L, k + int64_t(j) * L < k1, cj[j], vj[j]);
#pragma unroll
            for (int j = 0; j < G; j++)
            {
                // D == 1 only: with the slot defined on both paths the compiler keeps the schedule the scalar form had before
                // this pass served D outputs (f64, logistic row body: k_lin_rows 82 VGPRs and k_lin_rows_trial 83, 5 waves per
                // SIMD; without the line 96 and 97, and the trial form drops to 4 waves).  At D > 1 the kernels come out the
                // same without it (profiles/own_frame_kernel_resources.tsv)
                if constexpr (D == 1)
                    xj[j][0] = T(0);
                if (k + int64_t(j) * L < k1)
                    ld(int64_t(cj[j]), xj[j]);
            }
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
            const T value = lin_row_body<T>(obj, s, dz, r);
#pragma unroll
            for (int c = 0; c < D; c++)
                obj.w[r * D + c] = dz[c];
            obj.v[r] = value;
        }
    }
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_rows(const T* __restrict__ x, OBJ obj)
{
    lin_rows<T, LinCsr<T>>(obj, LinGather<T, lin_outputs<OBJ>>{x});
}

template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_lin_rows_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, OBJ obj)
{
    lin_rows<T, LinCsr<T>>(obj, LinGatherTrial<T, lin_outputs<OBJ>>{xp, d, step});
}

// ---------------------------------------------------------------- the column pass
// how every form's coordinate i with value xi starts: psi's value to fx, its derivative as the first term of the gradient
template <class T, class OBJ, class A>
__device__ __forceinline__ LinSum<T> lin_coord_start(const OBJ& obj, int64_t i, T xi, A& fx)
{
    LinSum<T> gv;
    if (OBJ::kCoord)
    {
        const T tx[1] = {xi};
        T tg[1];
        fx.add(obj.coord(tx, tg, i));
        gv.add(tg[0]);
    }
    return gv;
}

// what the sparse forms put between psi's term and the column's contributions: nothing
struct LinNoMid
{
    template <class S>
    __device__ __forceinline__ void operator()(S&) const
    {
    }
};

// coordinate i = j*D + c with value xi and column j's transposed entries [lo, hi): its gradient, returned; psi's value goes
// to fx.  The gradient is one running sum: psi's derivative, then whatever mid(gv) adds to it (the graph-regularised form's edge
// terms, linear_graph_kernels.cuh), then the column's contributions
template <class T, class OBJ, class A, class MID = LinNoMid>
__device__ __forceinline__ T lin_coord(const OBJ& obj, int64_t i, T xi, uint32_t lo, uint32_t hi, A& fx, MID mid = MID())
{
    constexpr int G = kLinGroup, D = lin_outputs<OBJ>;
    const int64_t j = i / D;
    const int c = int(i - j * D);
    LinSum<T> gv = lin_coord_start<T>(obj, i, xi, fx);
    mid(gv);
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
            gv.add(part[int64_t(q) * D + c]);
        return gv.value;
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
                gv.add(vj[t] * wj[t]);
    }
    return gv.value;
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

// what the families of the three forms share (own_frame.cuh): n coordinates, the frame's D = 1 ownership of one 16-byte
// pack of them, and every row's value as the extra pass
struct LinFamilyBase
{
    static constexpr int D = 1, U = kLinTrialU;
    template <class OBJ>
    static __device__ __forceinline__ int64_t nodes(const OBJ&, int64_t n)
    {
        return n;
    }
    template <class T, class OBJ, class A>
    static __device__ __forceinline__ void extra(const OBJ& obj, A& fx)
    {
        lin_row_values<T>(obj, fx);
    }
};

// the family of the two sparse forms: the transposed list at colptr.  SHARED false: a coordinate is a column and colptr
// holds the frame's offsets, n + 1 of them.  SHARED true: the D coordinates of a column walk one list and colptr has n / D + 1
// entries, so the family gives (lo, hi) per coordinate (kRange)
template <bool SHARED>
struct LinFamily : LinFamilyBase
{
    static constexpr bool kRange = SHARED;
    template <class OBJ>
    static __device__ __forceinline__ const uint32_t* off(const OBJ& obj)
    {
        return obj.colptr;
    }
    template <class OBJ>
    static __device__ __forceinline__ void range(const OBJ& obj, int64_t i, uint32_t& lo, uint32_t& hi)
    {
        const uint32_t* __restrict__ colptr = obj.colptr;
        const int64_t j = i / lin_outputs<OBJ>;
        lo = colptr[j];
        hi = colptr[j + 1];
    }
    template <class T, class OBJ, class LD, class A>
    static __device__ __forceinline__ void node(const OBJ& obj, int64_t i, const T (&xi)[1], uint32_t lo, uint32_t hi, LD, A& fx,
                                                T (&gi)[1])
    {
        gi[0] = lin_coord<T>(obj, i, xi[0], lo, hi, fx);
    }
};

// k_lin_eval, k_lin_trial, k_lin_b_eval, k_lin_b_dg_maxstep_trial
LBFGSX_OWN_KERNELS(k_lin, LinFamily<false>)

}  // namespace lbfgsx
