// lbfgspp_amd/csrc/grid_kernels.cuh -- the four evaluation kernels for a GRID objective
//     f(x) = sum over cells (r, c), 0 <= r < rows-1, 0 <= c < cols-1, of phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c)
// on a row-major rows x cols array x, n = rows*cols (include/lbfgsx.h, "grid objectives").
//
// k_grid_eval, k_grid_trial, k_grid_b_eval and k_grid_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval and
// k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion signal;
// launch_args.hpp serves all three families.  They are halo_eval and halo_trial (halo_frame.cuh) around GridFamily, at the
// end of this file: the frame holds the loops, the bounds, the sums and the tail's order; this file holds what a grid loads,
// its three windows, the cells of a pack and the position carried along the loop.  They are compiled at run time only
// (jit_objective.hip): OBJ is the struct generated around the caller's text for one cell,
//     int64_t rows, cols;   T term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col) const;
//
// Ownership.  The thread that owns coordinate j = r*cols + c writes grad[j] and adds the value of the cell whose origin is j
// (if there is one) to f's accumulator, once.  grad[j] is the sum of g[3] of cell (r-1, c-1), g[2] of cell (r-1, c), g[1] of
// cell (r, c-1) and g[0] of cell (r, c) -- those that exist, in this order (ascending flat index of the cell's origin),
// started from the first (no leading 0 +).  A thread owns the W coordinates of a 16-byte pack [b, b+W) of the flat array;
// thread 0 of block 0 also owns the coordinates past the last whole pack.
//
// The windows.  For its pack a thread holds three windows of W+2 values, x[b-cols-1 .. b-cols+W], x[b-1 .. b+W] and
// x[b+cols-1 .. b+cols+W], and evaluates the 2(W+1) cells whose origins are the first W+1 positions of the first two.  A cell
// with origin t exists iff t >= 0, t % cols < cols-1 and t / cols < rows-1; everything is uniform in the flat index, so a
// pack that straddles the end of a row is no special case.  Each window is a pack (its own, and the W values one row above
// and one row below) plus one value on either side, which comes from the neighbouring lane by the cross-lane moves of
// chain_window<T, 2> (chain_kernels.cuh), run by all 64 lanes; only wave-edge lanes and the lane with the last whole pack
// load a halo value from memory, with the pack's own loads.  When cols % W == 0 the rows above and below are aligned
// 16-byte loads of the packs cols/W away; otherwise they are element loads.  In the trial kernels every window value is
// xp + step*d -- the neighbouring lane's, or the same statement on loads of xp and d -- never a read of the x this launch
// writes.  No index below 0 or at or above n is loaded, and a cell that does not exist is not evaluated, so the text of a
// cell may read p0[i], p0[i+1], p0[i+cols] and p0[i+cols+1].
//
// (row, col) of a pack is found by one division per thread and launch and then advanced with the loop; a pack away from
// the four sides of the grid takes a path without existence tests.
#pragma once
#include "chain_kernels.cuh"

namespace lbfgsx {

struct GridPos
{
    int64_t row, col;
};
__device__ __forceinline__ GridPos grid_pos(int64_t flat, int64_t cols)
{
    const int64_t r = flat / cols;
    return {r, flat - r * cols};
}
// p += step / p -= step for a step with 0 <= step.col < cols
__device__ __forceinline__ void grid_advance(GridPos& p, const GridPos& step, int64_t cols)
{
    p.row += step.row;
    p.col += step.col;
    if (p.col >= cols)
    {
        p.col -= cols;
        p.row++;
    }
}
__device__ __forceinline__ void grid_retreat(GridPos& p, const GridPos& step, int64_t cols)
{
    p.row -= step.row;
    p.col -= step.col;
    if (p.col < 0)
    {
        p.col += cols;
        p.row--;
    }
}

// what a lane reads of one vector for the pack vi: the W values one row above (p[0]), its own pack (p[1]) and the W values
// one row below (p[2]), and per row the one halo value it has no neighbouring lane for (lane 0: to the left; lane 63 and the
// lane with the last whole pack: to the right).  Zero where the coordinate is not in [0, n) or the lane holds no pack.
template <class T>
struct GridLoads
{
    Pack<T> p[3];
    T edge[3][1];
};

template <class T>
__device__ __forceinline__ void grid_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t cols, bool aligned,
                                          GridLoads<T>& o)
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
            else if (aligned && lo >= 0 && lo + W <= n)
                o.p[r] = ldv(v, lo / W);
            else
            {
#pragma unroll
                for (int k = 0; k < W; k++)
                    if (lo + k >= 0 && lo + k < n)
                        o.p[r].e[k] = v[lo + k];
            }
            int64_t e = -1;
            if (lane == 0)
                e = lo - 1;
            else if (lane == 63 || vi + 1 >= nv)
                e = lo + W;
            if (e >= 0 && e < n)
                o.edge[r][0] = v[e];
        }
    }
}

// the cells whose origins are b + (PASS-1)*cols - 1 + s, s = 0 .. W: PASS 0 the row above the pack (the pack's coordinates
// are the cells' lower corners: g[2] and g[3]), PASS 1 the pack's own row (upper corners: g[0] and g[1]; the cells that
// start inside the pack add their value).  (row, col) is the position of b.  ALL: every one of them exists.
template <bool ALL, int PASS, class T, class OBJ, class A>
__device__ __forceinline__ void grid_cell_row(const OBJ& obj, int64_t b, int64_t row, int64_t col,
                                              const T (&top)[Vec16<T>::W + 2], const T (&bot)[Vec16<T>::W + 2], Pack<T>& g,
                                              bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W;
    constexpr int jl = PASS ? 0 : 2, jr = jl + 1;
    const int64_t cols = obj.cols, rows = obj.rows;
    const int64_t t = b + (PASS - 1) * cols - 1;
    int64_t r = row - 1 + PASS, c = col - 1;
    if (!ALL && c < 0)
    {
        c += cols;
        r--;
    }
#pragma unroll
    for (int s = 0; s <= W; s++)
    {
        if (ALL || (r >= 0 && c < cols - 1 && r < rows - 1))
        {
            const T tx[4] = {top[s], top[s + 1], bot[s], bot[s + 1]};
            T tg[4];
            const T v = obj.term(tx, tg, t + s, r, c);
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
        c++;
        if (!ALL && c == cols)
        {
            c = 0;
            r++;
        }
    }
}

// the gradient of the pack at vi (position pos) from its three windows, and the values of the cells that start inside it
template <class T, class OBJ, class A>
__device__ __forceinline__ void grid_pack(const OBJ& obj, int64_t vi, const GridPos& pos, const T (&up)[Vec16<T>::W + 2],
                                          const T (&mid)[Vec16<T>::W + 2], const T (&dn)[Vec16<T>::W + 2], Pack<T>& g, A& fx)
{
    constexpr int W = Vec16<T>::W;
    const int64_t b = vi * W;
    bool has[W];
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        has[k] = false;
        g.e[k] = T(0);
    }
    if (pos.row >= 1 && pos.row + 1 < obj.rows && pos.col >= 1 && pos.col + W + 1 <= obj.cols)
    {
        grid_cell_row<true, 0>(obj, b, pos.row, pos.col, up, mid, g, has, fx);
        grid_cell_row<true, 1>(obj, b, pos.row, pos.col, mid, dn, g, has, fx);
    }
    else
    {
        grid_cell_row<false, 0>(obj, b, pos.row, pos.col, up, mid, g, has, fx);
        grid_cell_row<false, 1>(obj, b, pos.row, pos.col, mid, dn, g, has, fx);
    }
}

// the three windows of the pack at vi from the values a lane holds (xv: x itself, or xp + step*d).  late(e): x at
// coordinate e from memory.  Called by all 64 lanes of the wave.
template <class T, class LATE>
__device__ __forceinline__ void grid_windows(const GridLoads<T>& xv, int64_t vi, int64_t nv, int64_t n, int64_t cols, LATE late,
                                             T (&up)[Vec16<T>::W + 2], T (&mid)[Vec16<T>::W + 2], T (&dn)[Vec16<T>::W + 2])
{
    constexpr int W = Vec16<T>::W;
    const int64_t b = vi * W;
    auto right = [&](int64_t e) { return (e >= 0 && e < n) ? late(e) : T(0); };
    chain_window<T, 2>(xv.p[0], xv.edge[0], vi, nv, [&](int j) { return right(b - cols + W + j); }, up);
    chain_window<T, 2>(xv.p[1], xv.edge[1], vi, nv, [&](int j) { return right(b + W + j); }, mid);
    chain_window<T, 2>(xv.p[2], xv.edge[2], vi, nv, [&](int j) { return right(b + cols + W + j); }, dn);
}

// a coordinate past the last whole pack (thread 0 of block 0): its gradient, returned, and the value of the cell that starts
// there.  ld(k) = x[k] for k in [0, n) -- from memory in the evaluation kernels, recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T grid_tail(const OBJ& obj, int64_t j, LD ld, A& fx)
{
    const int64_t cols = obj.cols, rows = obj.rows;
    const GridPos p = grid_pos(j, cols);
    T gi = T(0);
    bool has = false;
#pragma unroll
    for (int q = 0; q < 4; q++)  // cells (r-1, c-1), (r-1, c), (r, c-1), (r, c): ascending origin; j is their corner 3 - q
    {
        const int64_t r = p.row - (q < 2 ? 1 : 0), c = p.col - ((q & 1) ? 0 : 1);
        if (r >= 0 && c >= 0 && r < rows - 1 && c < cols - 1)
        {
            const int64_t t = r * cols + c;
            const T tx[4] = {ld(t), ld(t + 1), ld(t + cols), ld(t + cols + 1)};
            T tg[4];
            const T v = obj.term(tx, tg, t, r, c);
            gi = has ? gi + tg[3 - q] : tg[3 - q];
            has = true;
            if (q == 3)
                fx.add(v);
        }
    }
    return gi;
}

// the tile depth of the two trial kernels: a tile loads three rows of xp and of d (the chain kernels' 4 with one row)
constexpr int kGridTrialU = 2;

// the values of x = xp + step*d a lane holds, from its loads of xp and d
template <class T>
__device__ __forceinline__ void grid_axpy(const GridLoads<T>& xp, const GridLoads<T>& d, T step, GridLoads<T>& x)
{
    constexpr int W = Vec16<T>::W;
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            x.p[r].e[k] = xp.p[r].e[k] + step * d.p[r].e[k];
        x.edge[r][0] = xp.edge[r][0] + step * d.edge[r][0];
    }
}

// the frame's family (halo_frame.cuh): three rows of halo 1, and the (row, col) of a pack carried along the loop
template <class T, class OBJ>
struct GridFamily
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
        grid_load(v, vi, nv, n, obj.cols, obj.cols % W == 0, o);
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
        T up[W + 2], mid[W + 2], dn[W + 2];
        grid_windows(xv, vi, nv, n, obj.cols, ld, up, mid, dn);
        body(up, mid, dn);
    }
    template <class A>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T>& g, A& fx,
                                                const T (&up)[W + 2], const T (&mid)[W + 2], const T (&dn)[W + 2])
    {
        grid_pack(obj, vi, pos, up, mid, dn, g, fx);
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        return grid_tail<T>(obj, i, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_grid, halo_eval, halo_trial, GridFamily<T, OBJ>)

}  // namespace lbfgsx
