// lbfgspp_amd/csrc/grid_field_kernels.cuh -- the four evaluation kernels for a GRID FIELD objective
//     f(x) = sum over the cells (r, c) that exist of phi(u[r,c], u[r,c+1], u[r+1,c], u[r+1,c+1]; r, c),   + modulo the extent,
// on a row-major rows x cols grid whose nodes carry D = 1, 2 or 3 unknowns, u[r,c] = x[(r*cols + c)*D .. +D), n = rows*cols*D;
// cell existence, the mask obj.periodic and the wrapped corners are those of a periodic grid objective
// (periodic_grid_kernels.cuh; include/lbfgsx.h, "grid field objectives").  At D = 1 this is the periodic grid objective.
//
// k_gfield_eval, k_gfield_trial, k_gfield_b_eval and k_gfield_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion signal.
// They are halo_field_eval and halo_field_trial (halo_field_frame.cuh: halo_frame.cuh with P packs per thread) around
// GridFieldFamily, at the end of this file, which is PeriodicGridFamily with nodes of D values.  Compiled at run time only
// (jit_objective.hip): OBJ is the struct generated around the caller's text for one cell,
//     static constexpr int D;  int64_t rows, cols;  int periodic;
//     T term(const T (&x)[4 * D], T (&g)[4 * D], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const;
// x[k*D + d]: unknown d of corner k; i, j[k]: NODE indices (j[0] == i), the flat coordinate of x[k*D + d] is j[k]*D + d.
//
// Ownership.  A thread owns W = 16 / sizeof(T) consecutive NODES, that is the D consecutive 16-byte packs [vi*D, vi*D + D) of
// the flat array (the frame's P = D): a node never straddles two threads whatever D is, every own-row load and every store of
// x and g is an aligned 16-byte access, and over its D load instructions a wave covers 64*D*16 contiguous bytes.  The thread
// that owns node (r, c) writes, for every d, grad[(r,c), d] = g[3*D+d] of cell (r-1, c-1) + g[2*D+d] of (r-1, c) + g[D+d] of
// (r, c-1) + g[d] of (r, c) -- those that exist, in this order, started from the first, - modulo the extent on a periodic axis --
// and adds the value of cell (r, c) to f's accumulator.
//
// The windows are the grid form's three, of (W+2) nodes x D values: node s of a window holds its D values at [s*D, s*D + D).
// The halo nodes left and right come from the neighbouring lanes by cross-lane moves, D per side and row, run by all 64
// lanes; only wave-edge lanes and the lane with the last whole node pack load a halo node from memory.  The rows above and
// below are aligned 16-byte loads iff (cols*D) % W == 0 (then n % W == 0 too and a wrapped pack lies inside [0, n)), element
// loads otherwise; the row direction wraps in the loads, modulo rows*cols nodes.  A node pack that starts in column 0 or ends
// in column cols-1 replaces the 3*D halo values of that side by element loads through the frame's ld and then runs the same
// cells as every other pack; one that straddles the end of a row (cols % W != 0) goes node by node.  The nodes past the last
// whole node pack go through the frame's tail coordinate by coordinate; the cell's value is added for d = 0 only.
// The position carried along the loop is the grid's (row, col) of the first owned node; the frame's flat steps are in nodes.
// No index outside [0, n) is loaded.
#pragma once
#include "halo_field_frame.cuh"
#include "periodic_grid_kernels.cuh"

namespace lbfgsx {

// what a lane reads of one vector for the node pack vi: per row (above, own, below) the D packs of its W nodes and the one
// halo node it has no neighbouring lane for.  Zero where a node is outside the grid on an open axis or the lane holds no pack
template <class T, int D>
struct FieldLoads
{
    Pack<T> p[3][D];
    T edge[3][D];
};

// N: the nodes, n = N*D.  aligned: (cols*D) % W == 0.  wrap: the row direction is periodic
template <class T, int D>
__device__ __forceinline__ void gfield_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t cols, bool aligned,
                                            bool wrap, FieldLoads<T, D>& o)
{
    constexpr int W = Vec16<T>::W;
    const int lane = threadIdx.x & 63;
    const int64_t N = n / D, b = vi * W;
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
        const int64_t lo = b + (r - 1) * cols;  // the first of the row's W nodes
#pragma unroll
        for (int q = 0; q < D; q++)
        {
#pragma unroll
            for (int k = 0; k < W; k++)
                o.p[r][q].e[k] = T(0);
            o.edge[r][q] = T(0);
        }
        if (vi < nv)
        {
#pragma unroll
            for (int q = 0; q < D; q++)
            {
                const int64_t f = lo * D + q * W;  // -n <= f < 2n
                if (r == 1)
                    o.p[r][q] = ldv(v, vi * D + q);
                else if (aligned)  // f and n are multiples of W: the pack lies inside [0, n) or wholly outside
                {
                    const int64_t w = wrap_once(f, n);
                    if (wrap || w == f)
                        o.p[r][q] = ldv(v, w / W);
                }
                else
                {
#pragma unroll
                    for (int k = 0; k < W; k++)
                    {
                        const int64_t w = wrap_once(f + k, n);
                        if (wrap || w == f + k)
                            o.p[r][q].e[k] = v[w];
                    }
                }
            }
            if (lane == 0 || lane == 63 || vi + 1 >= nv)
            {
                const int64_t e = (lane == 0) ? lo - 1 : lo + W;
                const int64_t w = wrap_once(e, N);
                if (wrap || w == e)
                {
#pragma unroll
                    for (int d = 0; d < D; d++)
                        o.edge[r][d] = v[w * D + d];
                }
            }
        }
    }
}

// win[0 .. (W+2)*D) = the nodes b-1 .. b+W of one row around the lane's D packs: chain_window<T, 2> with nodes of D values.
// Called by all 64 lanes of the wave; late(d): unknown d of node b+W from memory (anything when that node does not exist)
template <class T, int D, class LATE>
__device__ __forceinline__ void gfield_window(const Pack<T> (&p)[D], const T (&edge)[D], int64_t vi, int64_t nv, LATE late,
                                              T (&win)[(Vec16<T>::W + 2) * D])
{
    constexpr int W = Vec16<T>::W;
    const int lane = threadIdx.x & 63;
    const bool mem_r = lane == 63 || vi + 1 >= nv;
#pragma unroll
    for (int d = 0; d < D; d++)
    {
        constexpr int last = (W - 1) * D;
        const T up = __shfl_up(p[(last + d) / W].e[(last + d) % W], 1, 64);
        const T dn = __shfl_down(p[d / W].e[d % W], 1, 64);
        win[d] = (lane == 0) ? edge[d] : up;
        win[(W + 1) * D + d] = mem_r ? edge[d] : dn;
    }
    if (lane == 0 && mem_r && vi < nv)
    {
#pragma unroll
        for (int d = 0; d < D; d++)
            win[(W + 1) * D + d] = late(d);
    }
#pragma unroll
    for (int m = 0; m < W * D; m++)
        win[D + m] = p[m / W].e[m % W];
}

// node t on its own (one past the last whole node pack, or one of a pack that straddles the end of a row): its up to four
// cells with every corner from ld(k) = x[k], 0 <= k < n; its D partial derivatives to gd and, if addf, the value of the cell
// that starts there to fx
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ void gfield_node(const OBJ& obj, int64_t t, LD ld, A& fx, T (&gd)[OBJ::D], bool addf)
{
    constexpr int D = OBJ::D;
    const int64_t cols = obj.cols, rows = obj.rows;
    const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
    const GridPos p = grid_pos(t, cols);
    const int64_t rr[3] = {p.row > 0 ? p.row - 1 : rows - 1, p.row, p.row + 1 < rows ? p.row + 1 : 0};
    const int64_t cc[3] = {p.col > 0 ? p.col - 1 : cols - 1, p.col, p.col + 1 < cols ? p.col + 1 : 0};
    const bool hr[2] = {p.row > 0 || pr, p.row + 1 < rows || pr}, hc[2] = {p.col > 0 || pc, p.col + 1 < cols || pc};
    bool has = false;
#pragma unroll
    for (int d = 0; d < D; d++)
        gd[d] = T(0);
#pragma unroll
    for (int q = 0; q < 4; q++)  // cells (r-1, c-1), (r-1, c), (r, c-1), (r, c): the node is their corner 3 - q
    {
        const int dr = q >> 1, dc = q & 1;
        if (hr[dr] && hc[dc])
        {
            const int64_t tj[4] = {rr[dr] * cols + cc[dc], rr[dr] * cols + cc[dc + 1], rr[dr + 1] * cols + cc[dc],
                                   rr[dr + 1] * cols + cc[dc + 1]};
            T tx[4 * D], tg[4 * D];
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
#pragma unroll
                for (int d = 0; d < D; d++)
                    tx[k * D + d] = ld(tj[k] * D + d);
            }
            const T v = obj.term(tx, tg, tj[0], rr[dr], cc[dc], tj);
#pragma unroll
            for (int d = 0; d < D; d++)
                gd[d] = has ? gd[d] + tg[(3 - q) * D + d] : tg[(3 - q) * D + d];
            has = true;
            if (q == 3 && addf)
                fx.add(v);
        }
    }
}

// pgrid_cell_row with nodes of D values: the cells whose origins are the first W+1 nodes of the window `top`, for a node pack
// at (row, col) that lies inside one row.  PASS 0: the row of cells above the pack (its nodes are their lower corners, slots 2
// and 3), PASS 1: the pack's own (upper corners, slots 0 and 1; the cells that start inside the pack add their value).  r0,
// r1: the rows of top and bot.  g: the pack's W*D partial derivatives, node-major
template <int PASS, class T, class OBJ, class A>
__device__ __forceinline__ void gfield_cell_row(const OBJ& obj, int64_t col, int64_t r0, int64_t r1,
                                                const T (&top)[(Vec16<T>::W + 2) * OBJ::D],
                                                const T (&bot)[(Vec16<T>::W + 2) * OBJ::D], T (&g)[Vec16<T>::W * OBJ::D],
                                                bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W, D = OBJ::D;
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
        T tx[4 * D], tg[4 * D];
#pragma unroll
        for (int d = 0; d < D; d++)
        {
            tx[d] = top[s * D + d];
            tx[D + d] = top[(s + 1) * D + d];
            tx[2 * D + d] = bot[s * D + d];
            tx[3 * D + d] = bot[(s + 1) * D + d];
        }
        const int64_t tj[4] = {b0 + c0, b0 + c1, b1 + c0, b1 + c1};
        const T v = obj.term(tx, tg, tj[0], r0, c0, tj);
        if (s < W)
        {
#pragma unroll
            for (int d = 0; d < D; d++)
                g[s * D + d] = has[s] ? g[s * D + d] + tg[jr * D + d] : tg[jr * D + d];
            has[s] = true;
        }
        if (s >= 1)
        {
#pragma unroll
            for (int d = 0; d < D; d++)
                g[(s - 1) * D + d] = has[s - 1] ? g[(s - 1) * D + d] + tg[jl * D + d] : tg[jl * D + d];
            has[s - 1] = true;
        }
        if (PASS == 1 && s >= 1)
            fx.add(v);
    }
}

// the frame's family (halo_field_frame.cuh): PeriodicGridFamily with D packs per thread
template <class T, class OBJ>
struct GridFieldFamily
{
    static constexpr int W = Vec16<T>::W, D = OBJ::D;
    static_assert(D >= 1 && D <= 3, "a node has D = 1, 2 or 3 unknowns");
    // at D = 1 the periodic grid form's depth; a deeper tile of D >= 2 does not fit the register file without scratch: per
    // vector and tile a lane holds 9*D values of loads (W = 2) and the 3*(W+2)*D values of the windows
    static constexpr int U = (D == 1) ? kGridTrialU : 1;
    static constexpr int P = D;
    typedef FieldLoads<T, D> Loads;
    typedef GridPos Pos;
    // flat: in nodes
    __device__ __forceinline__ static Pos pos(const OBJ& obj, int64_t flat) { return grid_pos(flat, obj.cols); }
    __device__ __forceinline__ static void advance(const OBJ& obj, Pos& p, const Pos& step) { grid_advance(p, step, obj.cols); }
    __device__ __forceinline__ static void retreat(const OBJ& obj, Pos& p, const Pos& step) { grid_retreat(p, step, obj.cols); }

    __device__ __forceinline__ static void load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, const OBJ& obj,
                                                Loads& o)
    {
        gfield_load<T, D>(v, vi, nv, n, obj.cols, (obj.cols * D) % W == 0, (obj.periodic & 2) != 0, o);
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
#pragma unroll
        for (int r = 0; r < 3; r++)
        {
#pragma unroll
            for (int q = 0; q < D; q++)
            {
#pragma unroll
                for (int k = 0; k < W; k++)
                    x.p[r][q].e[k] = xp.p[r][q].e[k] + step * d.p[r][q].e[k];
                x.edge[r][q] = xp.edge[r][q] + step * d.edge[r][q];
            }
        }
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l, int q) { return l.p[1][q]; }
    template <class LD, class BODY>
    __device__ __forceinline__ static void gather(const Loads& xv, int64_t vi, int64_t nv, int64_t n, const OBJ& obj, LD ld,
                                                  BODY body)
    {
        const int64_t cols = obj.cols, b = vi * W, N = n / D;
        const bool wrap = (obj.periodic & 2) != 0;
        auto right = [&](int64_t e, int d) {  // unknown d of node e, the node to the right of a row's W
            const int64_t w = wrap_once(e, N);
            return (wrap || w == e) ? ld(w * D + d) : T(0);
        };
        T up[(W + 2) * D], mid[(W + 2) * D], dn[(W + 2) * D];
        gfield_window<T, D>(xv.p[0], xv.edge[0], vi, nv, [&](int d) { return right(b - cols + W, d); }, up);
        gfield_window<T, D>(xv.p[1], xv.edge[1], vi, nv, [&](int d) { return right(b + W, d); }, mid);
        gfield_window<T, D>(xv.p[2], xv.edge[2], vi, nv, [&](int d) { return right(b + cols + W, d); }, dn);
        body(up, mid, dn, ld);
    }
    template <class A, class LD>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T> (&g)[D], A& fx,
                                                const T (&up)[(W + 2) * D], const T (&mid)[(W + 2) * D],
                                                const T (&dn)[(W + 2) * D], const LD& ld)
    {
        const int64_t cols = obj.cols, rows = obj.rows, row = pos.row, col = pos.col;
        T gw[W * D];  // node-major: the D packs' values in order
#pragma unroll
        for (int m = 0; m < W * D; m++)
            gw[m] = T(0);
        if (col + W > cols)  // the pack straddles the end of a row
        {
#pragma unroll 1
            for (int k = 0; k < W; k++)
            {
                T gd[D];
                gfield_node<T>(obj, vi * W + k, ld, fx, gd, true);
#pragma unroll
                for (int m = 0; m < W * D; m++)
                    gw[m] = (m / D == k) ? gd[m % D] : gw[m];
            }
        }
        else
        {
            const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0;
            const int64_t rr[3] = {row > 0 ? row - 1 : rows - 1, row, row + 1 < rows ? row + 1 : 0};
            T wu[(W + 2) * D], wm[(W + 2) * D], wd[(W + 2) * D];
#pragma unroll
            for (int s = 0; s < (W + 2) * D; s++)
            {
                wu[s] = up[s];
                wm[s] = mid[s];
                wd[s] = dn[s];
            }
            if (pc && col == 0)  // the nodes to the left of column 0 are the row's last
            {
#pragma unroll
                for (int d = 0; d < D; d++)
                {
                    wu[d] = ld((rr[0] * cols + cols - 1) * D + d);
                    wm[d] = ld((rr[1] * cols + cols - 1) * D + d);
                    wd[d] = ld((rr[2] * cols + cols - 1) * D + d);
                }
            }
            if (pc && col + W == cols)  // the nodes to the right of column cols-1 are the row's first
            {
#pragma unroll
                for (int d = 0; d < D; d++)
                {
                    wu[(W + 1) * D + d] = ld(rr[0] * cols * D + d);
                    wm[(W + 1) * D + d] = ld(rr[1] * cols * D + d);
                    wd[(W + 1) * D + d] = ld(rr[2] * cols * D + d);
                }
            }
            bool has[W];
#pragma unroll
            for (int k = 0; k < W; k++)
                has[k] = false;
            if (row > 0 || pr)
                gfield_cell_row<0>(obj, col, rr[0], rr[1], wu, wm, gw, has, fx);
            if (row + 1 < rows || pr)
                gfield_cell_row<1>(obj, col, rr[1], rr[2], wm, wd, gw, has, fx);
        }
#pragma unroll
        for (int m = 0; m < W * D; m++)
            g[m / W].e[m % W] = gw[m];
    }
    // coordinate i past the last whole node pack: unknown i % D of node i / D
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        const int64_t t = i / D;
        const int d = int(i - t * D);
        T gd[D];
        gfield_node<T>(obj, t, ld, fx, gd, d == 0);
        T gi = gd[0];
#pragma unroll
        for (int k = 1; k < D; k++)
            gi = (d == k) ? gd[k] : gi;
        return gi;
    }
};

LBFGSX_FRAME_KERNELS(k_gfield, halo_field_eval, halo_field_trial, GridFieldFamily<T, OBJ>)

}  // namespace lbfgsx
