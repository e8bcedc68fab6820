// lbfgspp_amd/csrc/grid_stencil_kernels.cuh -- the four evaluation kernels for a GRID STENCIL objective
//     f(x) = sum over the patches (r, c) that exist of phi(x[r+dr, c+dc], dr, dc = 0, 1, 2; r, c),   + modulo the extent,
// on a row-major rows x cols array x, n = rows*cols, rows >= 3 and cols >= 3; patch (r, c) exists iff (c < cols-2 or the
// column direction is periodic: bit 0 of obj.periodic) and (r < rows-2 or the row direction is: bit 1) (include/lbfgsx.h,
// "grid stencil objectives").
//
// k_stencil_eval, k_stencil_trial, k_stencil_b_eval and k_stencil_b_dg_maxstep_trial take the arguments of k_eval, k_trial,
// k_b_eval and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion
// signal.  They are halo_eval and halo_trial (halo_frame.cuh) around StencilFamily, at the end of this file.  Compiled at run
// time only (jit_objective.hip): OBJ is the struct generated around the caller's text for one patch,
//     int64_t rows, cols;  int periodic;
//     T term(const T (&x)[9], T (&g)[9], int64_t i, int64_t row, int64_t col, const int64_t (&j)[9]) const;
// x[3*dr + dc]: the node (row+dr, col+dc); j: the flat indices of the nine nodes, j[0] == i.
//
// Ownership and order.  The thread that owns coordinate (r, c) writes its grad, the sum of g[3*dr + dc] of patch (r-dr, c-dc)
// over dr = 2, 1, 0 (outer) and dc = 2, 1, 0 (inner) -- those that exist, in this order, started from the first, - modulo the
// extent on a periodic axis -- and adds the value of patch (r, c) to f's accumulator.
//
// The windows are five, x[b + (k-2)*cols - 2 .. b + (k-2)*cols + W + 2), k = 0 .. 4, for the pack [b, b+W): a pack of each of
// the rows r-2 .. r+2 with two values on either side, put together by the cross-lane moves of chain_window<T, 3>
// (chain_kernels.cuh) with all 64 lanes in them.
//   the row direction  wraps uniformly in the flat index, as in pgrid_load (periodic_grid_kernels.cuh): the node k rows above
//       t is (t - k*cols) mod n.  b +- cols and b +- 2*cols with the two halo values lie inside wrap_once's domain because
//       rows >= 3.  An aligned 16-byte load of the wrapped pack when cols % W == 0, element loads otherwise; where the row
//       direction is open nothing outside [0, n) is loaded.
//   the column direction  does not.  A pack that lies inside one row (col + W <= cols) keeps its windows and its 3(W+2)
//       patches, three passes (origin row r-2, r-1, r) of W+2 patches with origin columns col-2 .. col+W-1 in ascending order:
//       every halo slot whose column falls outside [0, cols) -- up to two on either side, in all five windows -- is replaced by
//       an element load of the wrapped node through the frame's ld (x[i], or xp[i] + step*d[i] in the trial kernels: never a
//       read of the x the launch writes).  With cols % W != 0 such a pack can start in column 1 or end in column cols-2, not
//       only in column 0 or cols-1.  On an open axis those patches do not exist and the slots are not read.
//   a pack that straddles the end of a row  (only when cols % W != 0) goes coordinate by coordinate through stencil_node, up
//       to nine patches with every value from ld; so do the n % W coordinates past the last whole pack.
// No index outside [0, n) is loaded, and a patch that does not exist is not evaluated.
#pragma once
#include "periodic_grid_kernels.cuh"

namespace lbfgsx {

// what a lane reads of one vector for the pack vi: the W values of the rows r-2 .. r+2 (p[2] its own pack) and per row the two
// halo values it has no neighbouring lane for (lane 0: to the left; lane 63 and the lane with the last whole pack: to the
// right).  Zero where the coordinate is not loaded or the lane holds no pack.
template <class T>
struct StencilLoads
{
    Pack<T> p[5];
    T edge[5][2];
};

// the tile depth of the two trial kernels: a tile loads five rows of xp and of d
constexpr int kStencilTrialU = 1;

// the row direction wrapped modulo n when wrap is set; with it clear, only what lies in [0, n)
template <class T>
__device__ __forceinline__ void stencil_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t cols,
                                             bool aligned, bool wrap, StencilLoads<T>& o)
{
    constexpr int W = Vec16<T>::W;
    const int lane = threadIdx.x & 63;
    const int64_t b = vi * W;
#pragma unroll
    for (int r = 0; r < 5; r++)
    {
        const int64_t lo = b + (r - 2) * cols;
#pragma unroll
        for (int k = 0; k < W; k++)
            o.p[r].e[k] = T(0);
        o.edge[r][0] = T(0);
        o.edge[r][1] = T(0);
        if (vi < nv)
        {
            if (r == 2)
                o.p[r] = ldv(v, vi);
            else if (aligned)  // lo and n are multiples of W: the pack lies inside [0, n) or wholly outside
            {
                const int64_t w = wrap_once(lo, n);
                if (wrap || w == lo)
                    o.p[r] = ldv(v, w / W);
            }
            else
            {
#pragma unroll
                for (int k = 0; k < W; k++)
                {
                    const int64_t w = wrap_once(lo + k, n);
                    if (wrap || w == lo + k)
                        o.p[r].e[k] = v[w];
                }
            }
            if (lane == 0 || lane == 63 || vi + 1 >= nv)
            {
#pragma unroll
                for (int j = 0; j < 2; j++)
                {
                    const int64_t e = (lane == 0) ? lo - 2 + j : lo + W + j;
                    const int64_t w = wrap_once(e, n);
                    if (wrap || w == e)
                        o.edge[r][j] = v[w];
                }
            }
        }
    }
}

// c mod cols for -cols <= c < 2*cols
__device__ __forceinline__ int64_t stencil_wrap(int64_t c, int64_t cols) { return c < 0 ? c + cols : (c >= cols ? c - cols : c); }

// coordinate i on its own (one past the last whole pack, or one of a pack that straddles the end of a row): its up to nine
// patches with every node from ld(k) = x[k], 0 <= k < n; its partial derivative, returned, and the value of the patch that
// starts there, added to fx
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T stencil_node(const OBJ& obj, int64_t i, LD ld, A& fx)
{
    const int64_t cols = obj.cols, rows = obj.rows;
    const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
    const GridPos p = grid_pos(i, cols);
    T gi = T(0);
    bool has = false;
#pragma unroll 1
    for (int q = 0; q < 9; q++)  // patches (r-2, c-2), (r-2, c-1), .. (r, c): the coordinate is their slot 8 - q
    {
        const int dr = 2 - q / 3, dc = 2 - q % 3;
        int64_t r0 = p.row - dr, c0 = p.col - dc;
        if ((r0 < 0 && !pr) || (c0 < 0 && !pc))
            continue;
        r0 = r0 < 0 ? r0 + rows : r0;
        c0 = c0 < 0 ? c0 + cols : c0;
        if ((r0 + 2 >= rows && !pr) || (c0 + 2 >= cols && !pc))
            continue;
        const int64_t rb[3] = {r0 * cols, stencil_wrap(r0 + 1, rows) * cols, stencil_wrap(r0 + 2, rows) * cols};
        const int64_t cc[3] = {c0, stencil_wrap(c0 + 1, cols), stencil_wrap(c0 + 2, cols)};
        int64_t tj[9];
        T tx[9], tg[9];
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            tj[k] = rb[k / 3] + cc[k % 3];
            tx[k] = ld(tj[k]);
        }
        const T v = obj.term(tx, tg, tj[0], r0, c0, tj);
        T mine = tg[0];
#pragma unroll
        for (int k = 1; k < 9; k++)
            mine = (k == 8 - q) ? tg[k] : mine;
        gi = has ? gi + mine : mine;
        has = true;
        if (q == 8)
            fx.add(v);
    }
    return gi;
}

// the W+2 patches with origin row r0 and origin columns col-2 .. col+W-1, for a pack at column col that lies inside one row:
// PASS 0, 1, 2 the patch rows whose origin is two rows above, one row above and in the pack's row, so that the pack's
// coordinates are the patches' nodes of row dr = 2 - PASS.  a, b, c: the windows of the rows r0, r1, r2 of the patch.  The
// patches that start inside the pack (PASS 2) add their value.
template <int PASS, class T, class OBJ, class A>
__device__ __forceinline__ void stencil_patch_row(const OBJ& obj, int64_t col, int64_t r0, int64_t r1, int64_t r2,
                                                  const T (&a)[Vec16<T>::W + 4], const T (&b)[Vec16<T>::W + 4],
                                                  const T (&c)[Vec16<T>::W + 4], Pack<T>& g, bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W;
    constexpr int jr = 3 * (2 - PASS);
    const int64_t cols = obj.cols;
    const bool pc = (obj.periodic & 1) != 0;
    const int64_t b0 = r0 * cols, b1 = r1 * cols, b2 = r2 * cols;
#pragma unroll
    for (int s = 0; s < W + 2; s++)
    {
        const int64_t oc = col - 2 + s;
        if (!pc && (oc < 0 || oc + 2 >= cols))
            continue;
        const int64_t c0 = stencil_wrap(oc, cols), c1 = stencil_wrap(oc + 1, cols), c2 = stencil_wrap(oc + 2, cols);
        const T tx[9] = {a[s], a[s + 1], a[s + 2], b[s], b[s + 1], b[s + 2], c[s], c[s + 1], c[s + 2]};
        const int64_t tj[9] = {b0 + c0, b0 + c1, b0 + c2, b1 + c0, b1 + c1, b1 + c2, b2 + c0, b2 + c1, b2 + c2};
        T tg[9];
        const T v = obj.term(tx, tg, tj[0], r0, c0, tj);
#pragma unroll
        for (int dc = 2; dc >= 0; dc--)
        {
            const int k = s + dc - 2;  // the pack's coordinate that tg[jr + dc] belongs to
            if (k >= 0 && k < W)
            {
                g.e[k] = has[k] ? g.e[k] + tg[jr + dc] : tg[jr + dc];
                has[k] = true;
            }
        }
        if (PASS == 2 && s >= 2)
            fx.add(v);
    }
}

// the frame's family (halo_frame.cuh): five rows of halo 2, the (row, col) of a pack carried along the loop, the frame's ld
// behind the windows, and a pack that patches the column seam
template <class T, class OBJ>
struct StencilFamily
{
    static constexpr int W = Vec16<T>::W;
    static constexpr int U = kStencilTrialU;
    typedef StencilLoads<T> Loads;
    typedef GridPos Pos;
    __device__ __forceinline__ static Pos pos(const OBJ& obj, int64_t flat) { return grid_pos(flat, obj.cols); }
    __device__ __forceinline__ static void advance(const OBJ& obj, Pos& p, const Pos& step) { grid_advance(p, step, obj.cols); }
    __device__ __forceinline__ static void retreat(const OBJ& obj, Pos& p, const Pos& step) { grid_retreat(p, step, obj.cols); }

    __device__ __forceinline__ static void load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, const OBJ& obj,
                                                Loads& o)
    {
        stencil_load(v, vi, nv, n, obj.cols, obj.cols % W == 0, (obj.periodic & 2) != 0, o);
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
#pragma unroll
        for (int r = 0; r < 5; r++)
        {
#pragma unroll
            for (int k = 0; k < W; k++)
                x.p[r].e[k] = xp.p[r].e[k] + step * d.p[r].e[k];
            x.edge[r][0] = xp.edge[r][0] + step * d.edge[r][0];
            x.edge[r][1] = xp.edge[r][1] + step * d.edge[r][1];
        }
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l) { return l.p[2]; }
    template <class LD, class BODY>
    __device__ __forceinline__ static void gather(const Loads& xv, int64_t vi, int64_t nv, int64_t n, const OBJ& obj, LD ld,
                                                  BODY body)
    {
        const int64_t cols = obj.cols, b = vi * W;
        const bool wrap = (obj.periodic & 2) != 0;
        auto right = [&](int64_t e) {
            const int64_t w = wrap_once(e, n);
            return (wrap || w == e) ? ld(w) : T(0);
        };
        T w0[W + 4], w1[W + 4], w2[W + 4], w3[W + 4], w4[W + 4];
        chain_window<T, 3>(xv.p[0], xv.edge[0], vi, nv, [&](int j) { return right(b - 2 * cols + W + j); }, w0);
        chain_window<T, 3>(xv.p[1], xv.edge[1], vi, nv, [&](int j) { return right(b - cols + W + j); }, w1);
        chain_window<T, 3>(xv.p[2], xv.edge[2], vi, nv, [&](int j) { return right(b + W + j); }, w2);
        chain_window<T, 3>(xv.p[3], xv.edge[3], vi, nv, [&](int j) { return right(b + cols + W + j); }, w3);
        chain_window<T, 3>(xv.p[4], xv.edge[4], vi, nv, [&](int j) { return right(b + 2 * cols + W + j); }, w4);
        body(w0, w1, w2, w3, w4, ld);
    }
    template <class A, class LD>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T>& g, A& fx,
                                                const T (&w0)[W + 4], const T (&w1)[W + 4], const T (&w2)[W + 4],
                                                const T (&w3)[W + 4], const T (&w4)[W + 4], const LD& ld)
    {
        const int64_t cols = obj.cols, rows = obj.rows, row = pos.row, col = pos.col;
        if (col + W > cols)  // the pack straddles the end of a row
        {
#pragma unroll
            for (int kk = 0; kk < W; kk++)
                g.e[kk] = T(0);
#pragma unroll 1
            for (int k = 0; k < W; k++)
            {
                const T gi = stencil_node<T>(obj, vi * W + k, ld, fx);
#pragma unroll
                for (int kk = 0; kk < W; kk++)
                    g.e[kk] = (kk == k) ? gi : g.e[kk];
            }
            return;
        }
        const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
        // the rows of the five windows, wrapped whether the row direction is periodic or not: always inside the grid
        const int64_t rr[5] = {stencil_wrap(row - 2, rows), stencil_wrap(row - 1, rows), row, stencil_wrap(row + 1, rows),
                               stencil_wrap(row + 2, rows)};
        T v0[W + 4], v1[W + 4], v2[W + 4], v3[W + 4], v4[W + 4];
#pragma unroll
        for (int s = 0; s < W + 4; s++)
        {
            v0[s] = w0[s];
            v1[s] = w1[s];
            v2[s] = w2[s];
            v3[s] = w3[s];
            v4[s] = w4[s];
        }
        if (pc && (col < 2 || col + W + 2 > cols))  // halo slots across the column seam: the wrapped nodes of the same rows
        {
#pragma unroll
            for (int t = 0; t < 4; t++)
            {
                const int s = t < 2 ? t : W + t;  // slots 0, 1 and W+2, W+3
                const int64_t cc = col - 2 + s;
                if (cc < 0 || cc >= cols)
                {
                    const int64_t cw = stencil_wrap(cc, cols);
                    v0[s] = ld(rr[0] * cols + cw);
                    v1[s] = ld(rr[1] * cols + cw);
                    v2[s] = ld(rr[2] * cols + cw);
                    v3[s] = ld(rr[3] * cols + cw);
                    v4[s] = ld(rr[4] * cols + cw);
                }
            }
        }
        bool has[W];
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            has[k] = false;
            g.e[k] = T(0);
        }
        // a patch row with origin row o exists iff the row direction is periodic or 0 <= o and o + 2 < rows
        if (pr || (row >= 2 && row < rows))
            stencil_patch_row<0>(obj, col, rr[0], rr[1], rr[2], v0, v1, v2, g, has, fx);
        if (pr || (row >= 1 && row + 1 < rows))
            stencil_patch_row<1>(obj, col, rr[1], rr[2], rr[3], v1, v2, v3, g, has, fx);
        if (pr || row + 2 < rows)
            stencil_patch_row<2>(obj, col, rr[2], rr[3], rr[4], v2, v3, v4, g, has, fx);
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        return stencil_node<T>(obj, i, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_stencil, halo_eval, halo_trial, StencilFamily<T, OBJ>)

}  // namespace lbfgsx
