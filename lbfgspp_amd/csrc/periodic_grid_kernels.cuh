// lbfgspp_amd/csrc/periodic_grid_kernels.cuh -- the four evaluation kernels for a PERIODIC GRID objective
//     f(x) = sum over the cells (r, c) that exist of phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c),   + modulo the extent,
// on a row-major rows x cols array x, n = rows*cols; cell (r, c) exists iff (c < cols-1 or the column direction is periodic:
// bit 0 of obj.periodic) and (r < rows-1 or the row direction is: bit 1) (include/lbfgsx.h, "periodic grid and volume
// objectives").  With the mask 0 this is the grid objective of grid_kernels.cuh.
//
// k_pgrid_eval, k_pgrid_trial, k_pgrid_b_eval and k_pgrid_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion signal.
// They are halo_eval and halo_trial (halo_frame.cuh) around PeriodicGridFamily, at the end of this file, which is GridFamily
// with other loads and another pack.  Compiled at run time only (jit_objective.hip): OBJ is the struct generated around the
// caller's text for one cell,
//     int64_t rows, cols;  int periodic;
//     T term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const;
// j: the flat indices of the cell's four corners, j[0] == i; at a seam they are not i+1, i+cols and i+cols+1.
//
// Ownership and order are the grid form's: the thread that owns coordinate (r, c) writes its grad, the sum of g[3] of cell
// (r-1, c-1), g[2] of (r-1, c), g[1] of (r, c-1) and g[0] of (r, c) -- those that exist, in this order, started from the first,
// - modulo the extent on a periodic axis -- and adds the value of cell (r, c) to f's accumulator.
//
// The windows are the grid form's three, x[b-cols-1 .. b-cols+W], x[b-1 .. b+W] and x[b+cols-1 .. b+cols+W], put together by
// the same cross-lane moves with all 64 lanes in them.  What differs:
//   the row direction  wraps uniformly in the flat index: the node above t is (t - cols) mod n, the node below (t + cols)
//       mod n, for a pack that straddles the end of a row too.  The loads do that (pgrid_load): an aligned 16-byte load of
//       the wrapped pack when cols % W == 0 (then n % W == 0 too), element loads of the wrapped coordinates otherwise.  Where
//       the row direction is open they load what grid_load loads.
//   the column direction  does not: the left neighbour of a node in column 0 is t - 1 + cols, the right neighbour of one in
//       column cols-1 is t + 1 - cols.  A pack that lies inside one row (col + W <= cols) keeps its windows and its 2(W+1)
//       cells: when it starts in column 0 the three left-hand halo values, when it ends in column cols-1 the three
//       right-hand ones are replaced by element loads through the frame's ld (x[i], or xp[i] + step*d[i] in the trial
//       kernels: never a read of the x the launch writes), which the frame hands to the pack as the last of the family's
//       "windows".  Those are two packs per row; every pack runs the same cells, so a wave with a seam pack in it runs
//       nothing twice.  Only the first and the last cell of a row of cells and a whole row of cells have an existence test.
//   a pack that straddles the end of a row  (only when cols % W != 0) goes coordinate by coordinate through the tail's
//       function, nine element loads by ld each.
// No index outside [0, n) is loaded.
#pragma once
#include "grid_kernels.cuh"

namespace lbfgsx {

// i mod n for -n <= i < 2n
__device__ __forceinline__ int64_t wrap_once(int64_t i, int64_t n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// grid_load with the row direction wrapped modulo n when wrap is set; with it clear, exactly grid_load's loads
template <class T>
__device__ __forceinline__ void pgrid_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t cols, bool aligned,
                                           bool wrap, GridLoads<T>& o)
{
    constexpr int W = Vec16<T>::W;
    const int lane = threadIdx.x & 63;
    const int64_t b = vi * W;
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
        const int64_t lo = b + (r - 1) * cols;
#pragma unroll
        for (int k = 0; k < W; k++)
            o.p[r].e[k] = T(0);
        o.edge[r][0] = T(0);
        if (vi < nv)
        {
            if (r == 1)
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
                const int64_t e = (lane == 0) ? lo - 1 : lo + W;
                const int64_t w = wrap_once(e, n);
                if (wrap || w == e)
                    o.edge[r][0] = v[w];
            }
        }
    }
}

// coordinate i on its own (one past the last whole pack, or one of a pack that straddles the end of a row): its up to four
// cells with every corner from ld(k) = x[k], 0 <= k < n; its partial derivative, returned, and the value of the cell that
// starts there, added to fx
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T pgrid_node(const OBJ& obj, int64_t i, LD ld, A& fx)
{
    const int64_t cols = obj.cols, rows = obj.rows;
    const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
    const GridPos p = grid_pos(i, cols);
    const int64_t rr[3] = {p.row > 0 ? p.row - 1 : rows - 1, p.row, p.row + 1 < rows ? p.row + 1 : 0};
    const int64_t cc[3] = {p.col > 0 ? p.col - 1 : cols - 1, p.col, p.col + 1 < cols ? p.col + 1 : 0};
    const bool hr[2] = {p.row > 0 || pr, p.row + 1 < rows || pr}, hc[2] = {p.col > 0 || pc, p.col + 1 < cols || pc};
    T gi = T(0);
    bool has = false;
#pragma unroll
    for (int q = 0; q < 4; q++)  // cells (r-1, c-1), (r-1, c), (r, c-1), (r, c): the coordinate is their corner 3 - q
    {
        const int dr = q >> 1, dc = q & 1;
        if (hr[dr] && hc[dc])
        {
            const int64_t tj[4] = {rr[dr] * cols + cc[dc], rr[dr] * cols + cc[dc + 1], rr[dr + 1] * cols + cc[dc],
                                   rr[dr + 1] * cols + cc[dc + 1]};
            const T tx[4] = {ld(tj[0]), ld(tj[1]), ld(tj[2]), ld(tj[3])};
            T tg[4];
            const T v = obj.term(tx, tg, tj[0], rr[dr], cc[dc], tj);
            gi = has ? gi + tg[3 - q] : tg[3 - q];
            has = true;
            if (q == 3)
                fx.add(v);
        }
    }
    return gi;
}

// the cells whose origins are the first W+1 positions of the window `top`, for a pack at (row, col) that lies inside one row:
// PASS 0 the row of cells above the pack (the pack's coordinates are their lower corners: g[2] and g[3]), PASS 1 the pack's
// own (upper corners: g[0] and g[1]; the cells that start inside the pack add their value).  r0, r1: the rows of top and bot
template <int PASS, class T, class OBJ, class A>
__device__ __forceinline__ void pgrid_cell_row(const OBJ& obj, int64_t col, int64_t r0, int64_t r1, const T (&top)[Vec16<T>::W + 2],
                                               const T (&bot)[Vec16<T>::W + 2], Pack<T>& g, bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W;
    constexpr int jl = PASS ? 0 : 2, jr = jl + 1;
    const int64_t cols = obj.cols;
    const bool pc = (obj.periodic & 1) != 0;
    const int64_t b0 = r0 * cols, b1 = r1 * cols;
#pragma unroll
    for (int s = 0; s <= W; s++)
    {
        if ((s == 0 && !(col > 0 || pc)) || (s == W && !(col + W < cols || pc)))
            continue;
        const int64_t c0 = (s == 0 && col == 0) ? cols - 1 : col - 1 + s;
        const int64_t c1 = (s == W && col + W == cols) ? 0 : col + s;
        const T tx[4] = {top[s], top[s + 1], bot[s], bot[s + 1]};
        const int64_t tj[4] = {b0 + c0, b0 + c1, b1 + c0, b1 + c1};
        T tg[4];
        const T v = obj.term(tx, tg, tj[0], r0, c0, tj);
        if (s < W)
        {
            g.e[s] = has[s] ? g.e[s] + tg[jr] : tg[jr];
            has[s] = true;
        }
        if (s >= 1)
        {
            g.e[s - 1] = has[s - 1] ? g.e[s - 1] + tg[jl] : tg[jl];
            has[s - 1] = true;
        }
        if (PASS == 1 && s >= 1)
            fx.add(v);
    }
}

// the frame's family (halo_frame.cuh): GridFamily's loads with the row direction wrapped, its windows with the frame's ld
// behind them, and a pack that patches the column seam
template <class T, class OBJ>
struct PeriodicGridFamily
{
    static constexpr int W = Vec16<T>::W;
    static constexpr int U = kGridTrialU;
    typedef GridLoads<T> Loads;
    typedef GridPos Pos;
    __device__ __forceinline__ static Pos pos(const OBJ& obj, int64_t flat) { return grid_pos(flat, obj.cols); }
    __device__ __forceinline__ static void advance(const OBJ& obj, Pos& p, const Pos& step) { grid_advance(p, step, obj.cols); }
    __device__ __forceinline__ static void retreat(const OBJ& obj, Pos& p, const Pos& step) { grid_retreat(p, step, obj.cols); }

    __device__ __forceinline__ static void load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, const OBJ& obj,
                                                Loads& o)
    {
        pgrid_load(v, vi, nv, n, obj.cols, obj.cols % W == 0, (obj.periodic & 2) != 0, o);
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
        grid_axpy(xp, d, step, x);
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l) { return l.p[1]; }
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
        T up[W + 2], mid[W + 2], dn[W + 2];
        chain_window<T, 2>(xv.p[0], xv.edge[0], vi, nv, [&](int j) { return right(b - cols + W + j); }, up);
        chain_window<T, 2>(xv.p[1], xv.edge[1], vi, nv, [&](int j) { return right(b + W + j); }, mid);
        chain_window<T, 2>(xv.p[2], xv.edge[2], vi, nv, [&](int j) { return right(b + cols + W + j); }, dn);
        body(up, mid, dn, ld);
    }
    template <class A, class LD>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T>& g, A& fx,
                                                const T (&up)[W + 2], const T (&mid)[W + 2], const T (&dn)[W + 2], const LD& ld)
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
                const T gi = pgrid_node<T>(obj, vi * W + k, ld, fx);
#pragma unroll
                for (int kk = 0; kk < W; kk++)
                    g.e[kk] = (kk == k) ? gi : g.e[kk];
            }
            return;
        }
        const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
        const int64_t rr[3] = {row > 0 ? row - 1 : rows - 1, row, row + 1 < rows ? row + 1 : 0};
        T wu[W + 2], wm[W + 2], wd[W + 2];
#pragma unroll
        for (int s = 0; s < W + 2; s++)
        {
            wu[s] = up[s];
            wm[s] = mid[s];
            wd[s] = dn[s];
        }
        if (pc && col == 0)  // the nodes to the left of column 0 are the row's last
        {
            wu[0] = ld(rr[0] * cols + cols - 1);
            wm[0] = ld(rr[1] * cols + cols - 1);
            wd[0] = ld(rr[2] * cols + cols - 1);
        }
        if (pc && col + W == cols)  // the nodes to the right of column cols-1 are the row's first
        {
            wu[W + 1] = ld(rr[0] * cols);
            wm[W + 1] = ld(rr[1] * cols);
            wd[W + 1] = ld(rr[2] * cols);
        }
        bool has[W];
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            has[k] = false;
            g.e[k] = T(0);
        }
        if (row > 0 || pr)
            pgrid_cell_row<0>(obj, col, rr[0], rr[1], wu, wm, g, has, fx);
        if (row + 1 < rows || pr)
            pgrid_cell_row<1>(obj, col, rr[1], rr[2], wm, wd, g, has, fx);
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        return pgrid_node<T>(obj, i, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_pgrid, halo_eval, halo_trial, PeriodicGridFamily<T, OBJ>)

}  // namespace lbfgsx
