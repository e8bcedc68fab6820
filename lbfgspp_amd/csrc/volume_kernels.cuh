// lbfgspp_amd/csrc/volume_kernels.cuh -- the four evaluation kernels for a VOLUME objective
//     f(x) = sum over cells (s, r, c), 0 <= s < slabs-1, 0 <= r < rows-1, 0 <= c < cols-1, of phi(x[8]; s, r, c),
//     x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc]
// on a slab-major slabs x rows x cols array x, n = slabs*rows*cols (include/lbfgsx.h, "volume objectives").
//
// k_volume_eval, k_volume_trial, k_volume_b_eval and k_volume_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion signal;
// launch_args.hpp serves all the families.  They are halo_eval and halo_trial (halo_frame.cuh) around VolumeFamily, at the end
// of this file, which is GridFamily (grid_kernels.cuh) with one more direction.  They are compiled at run time only
// (jit_objective.hip): OBJ is the struct generated around the caller's text for one cell,
//     int64_t slabs, rows, cols;   T term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col) const;
//
// Ownership.  The thread that owns coordinate j = (s*rows + r)*cols + c writes grad[j] and adds the value of the cell whose
// origin is j (if there is one) to f's accumulator, once.  grad[j] is the sum of g[7] of cell (s-1, r-1, c-1), g[6] of
// (s-1, r-1, c), g[5] of (s-1, r, c-1), g[4] of (s-1, r, c), g[3] of (s, r-1, c-1), g[2] of (s, r-1, c), g[1] of (s, r, c-1)
// and g[0] of (s, r, c) -- those that exist, in this order (ascending flat index of the cell's origin), started from the first
// (no leading 0 +).  A thread owns the W coordinates of a 16-byte pack [b, b+W) of the flat array; thread 0 of block 0 also
// owns the coordinates past the last whole pack.
//
// The windows.  With rc = rows*cols, a thread holds nine windows of W+2 values for its pack,
//     win[ds][dr] = x[b + (ds-1)*rc + (dr-1)*cols - 1 .. + W],   ds, dr = 0, 1, 2,
// and evaluates the 4(W+1) cells whose origins are the first W+1 positions of the four windows with ds, dr < 2, in four passes
// (slab above or own) x (row above or own).  A cell with flat origin t exists iff t >= 0 and the position (s, r, c) of t has
// s < slabs-1, r < rows-1 and c < cols-1; everything is uniform in the flat index, so a pack that straddles the end of a row
// or of a slab is no special case.  Each window is a pack (the thread's own, or the W values some rows and slabs away) plus
// one value on either side, which comes from the neighbouring lane by the cross-lane moves of chain_window<T, 2>
// (chain_kernels.cuh), run by all 64 lanes; only wave-edge lanes and the lane with the last whole pack load a halo value
// from memory, with the pack's own loads.  The packs one row away are aligned 16-byte loads when cols % W == 0, those one
// slab away when rc % W == 0, those one row and one slab away when both hold; otherwise they are element loads, each
// coordinate checked against [0, n).  In the trial kernels every window value is xp + step*d -- the neighbouring lane's, or
// the same statement on loads of xp and d -- never a read of the x this launch writes.  No index below 0 or at or above n
// is loaded, and a cell that does not exist is not evaluated, so the text of a cell may read p0 at its eight corners.
//
// (slab, row, col) of a pack is found by two divisions per thread and launch and then advanced with the loop; a pack away
// from the six faces of the volume takes a path without existence tests.
#pragma once
#include "grid_kernels.cuh"

namespace lbfgsx {

struct VolumePos
{
    int64_t slab, row, col;
};
__device__ __forceinline__ VolumePos volume_pos(int64_t flat, int64_t rows, int64_t cols)
{
    const int64_t q = flat / cols;
    const int64_t s = q / rows;
    return {s, q - s * rows, flat - q * cols};
}
// p += step / p -= step for a step with 0 <= step.col < cols and 0 <= step.row < rows
__device__ __forceinline__ void volume_advance(VolumePos& p, const VolumePos& step, int64_t rows, int64_t cols)
{
    p.slab += step.slab;
    p.row += step.row;
    p.col += step.col;
    if (p.col >= cols)
    {
        p.col -= cols;
        p.row++;
    }
    if (p.row >= rows)
    {
        p.row -= rows;
        p.slab++;
    }
}
__device__ __forceinline__ void volume_retreat(VolumePos& p, const VolumePos& step, int64_t rows, int64_t cols)
{
    p.slab -= step.slab;
    p.row -= step.row;
    p.col -= step.col;
    if (p.col < 0)
    {
        p.col += cols;
        p.row--;
    }
    if (p.row < 0)
    {
        p.row += rows;
        p.slab--;
    }
}

// what a lane reads of one vector for the pack vi: p[ds][dr] the W values (ds-1) slabs and (dr-1) rows away (p[1][1] its
// own pack), and per pack the one halo value it has no neighbouring lane for (lane 0: to the left; lane 63 and the lane with
// the last whole pack: to the right).  Zero where the coordinate is not in [0, n) or the lane holds no pack.
template <class T>
struct VolumeLoads
{
    Pack<T> p[3][3];
    T edge[3][3][1];
};

template <class T>
__device__ __forceinline__ void volume_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t rc, int64_t cols,
                                            bool slab_aligned, bool row_aligned, VolumeLoads<T>& o)
{
    constexpr int W = Vec16<T>::W;
    const int lane = threadIdx.x & 63;
    const int64_t b = vi * W;
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int r = 0; r < 3; r++)
        {
            const int64_t lo = b + (s - 1) * rc + (r - 1) * cols;
            const bool aligned = (s == 1 || slab_aligned) && (r == 1 || row_aligned);
#pragma unroll
            for (int k = 0; k < W; k++)
                o.p[s][r].e[k] = T(0);
            o.edge[s][r][0] = T(0);
            if (vi < nv)
            {
                if (s == 1 && r == 1)
                    o.p[s][r] = ldv(v, vi);
                else if (aligned && lo >= 0 && lo + W <= n)
                    o.p[s][r] = ldv(v, lo / W);
                else
                {
#pragma unroll
                    for (int k = 0; k < W; k++)
                        if (lo + k >= 0 && lo + k < n)
                            o.p[s][r].e[k] = v[lo + k];
                }
                int64_t e = -1;
                if (lane == 0)
                    e = lo - 1;
                else if (lane == 63 || vi + 1 >= nv)
                    e = lo + W;
                if (e >= 0 && e < n)
                    o.edge[s][r][0] = v[e];
            }
        }
}

// the cells whose origins are b + (PS-1)*rc + (PR-1)*cols - 1 + s, s = 0 .. W: PS 0 the slab above the pack, 1 its own; PR 0
// the row above, 1 its own.  The pack's coordinates are the cells' corners 4*(1-PS) + 2*(1-PR) + dc; the cells of its own
// slab and row that start inside the pack add their value.  w<ds><dr>: the windows of the cells' slab (ds 0) and the one
// below (ds 1), of the cells' row (dr 0) and the one below (dr 1).  pos is the position of b.  ALL: every cell exists.
template <bool ALL, int PS, int PR, class T, class OBJ, class A>
__device__ __forceinline__ void volume_cell_row(const OBJ& obj, int64_t b, const VolumePos& pos,
                                                const T (&w00)[Vec16<T>::W + 2], const T (&w01)[Vec16<T>::W + 2],
                                                const T (&w10)[Vec16<T>::W + 2], const T (&w11)[Vec16<T>::W + 2], Pack<T>& g,
                                                bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W;
    constexpr int jl = 4 * (1 - PS) + 2 * (1 - PR), jr = jl + 1;
    const int64_t cols = obj.cols, rows = obj.rows, slabs = obj.slabs;
    const int64_t t = b + (PS - 1) * (rows * cols) + (PR - 1) * cols - 1;
    int64_t sl = pos.slab - 1 + PS, r = pos.row - 1 + PR, c = pos.col - 1;
    if (!ALL)
    {
        if (c < 0)
        {
            c += cols;
            r--;
        }
        if (r < 0)
        {
            r += rows;
            sl--;
        }
    }
#pragma unroll
    for (int s = 0; s <= W; s++)
    {
        if (ALL || (sl >= 0 && sl < slabs - 1 && r < rows - 1 && c < cols - 1))
        {
            const T tx[8] = {w00[s], w00[s + 1], w01[s], w01[s + 1], w10[s], w10[s + 1], w11[s], w11[s + 1]};
            T tg[8];
            const T v = obj.term(tx, tg, t + s, sl, r, c);
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
            if (PS == 1 && PR == 1 && s >= 1)
                fx.add(v);
        }
        c++;
        if (!ALL && c == cols)
        {
            c = 0;
            r++;
            if (r == rows)
            {
                r = 0;
                sl++;
            }
        }
    }
}

// a coordinate past the last whole pack (thread 0 of block 0): its gradient, returned, and the value of the cell that starts
// there.  ld(k) = x[k] for k in [0, n) -- from memory in the evaluation kernels, recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T volume_tail(const OBJ& obj, int64_t j, LD ld, A& fx)
{
    const int64_t cols = obj.cols, rows = obj.rows, slabs = obj.slabs, rc = rows * cols;
    const VolumePos p = volume_pos(j, rows, cols);
    T gi = T(0);
    bool has = false;
#pragma unroll 1
    for (int q = 0; q < 8; q++)  // cells (s-1, r-1, c-1) .. (s, r, c): ascending origin; j is their corner 7 - q
    {
        const int64_t sl = p.slab - ((q & 4) ? 0 : 1), r = p.row - ((q & 2) ? 0 : 1), c = p.col - ((q & 1) ? 0 : 1);
        if (sl >= 0 && r >= 0 && c >= 0 && sl < slabs - 1 && r < rows - 1 && c < cols - 1)
        {
            const int64_t t = (sl * rows + r) * cols + c;
            const T tx[8] = {ld(t),      ld(t + 1),      ld(t + cols),      ld(t + cols + 1),
                             ld(t + rc), ld(t + rc + 1), ld(t + rc + cols), ld(t + rc + cols + 1)};
            T tg[8];
            const T v = obj.term(tx, tg, t, sl, r, c);
            T mine = tg[0];
#pragma unroll
            for (int k = 1; k < 8; k++)
                mine = (k == 7 - q) ? tg[k] : mine;
            gi = has ? gi + mine : mine;
            has = true;
            if (q == 7)
                fx.add(v);
        }
    }
    return gi;
}

// the tile depth of the two trial kernels: a tile loads nine packs of xp and of d per lane
constexpr int kVolumeTrialU = 1;

// the frame's family (halo_frame.cuh): three slabs of three rows of halo 1, and the (slab, row, col) of a pack carried along
// the loop
template <class T, class OBJ>
struct VolumeFamily
{
    static constexpr int W = Vec16<T>::W;
    static constexpr int U = kVolumeTrialU;
    typedef VolumeLoads<T> Loads;
    typedef VolumePos Pos;
    typedef T Win[W + 2];
    __device__ __forceinline__ static Pos pos(const OBJ& obj, int64_t flat) { return volume_pos(flat, obj.rows, obj.cols); }
    __device__ __forceinline__ static void advance(const OBJ& obj, Pos& p, const Pos& step)
    {
        volume_advance(p, step, obj.rows, obj.cols);
    }
    __device__ __forceinline__ static void retreat(const OBJ& obj, Pos& p, const Pos& step)
    {
        volume_retreat(p, step, obj.rows, obj.cols);
    }

    __device__ __forceinline__ static void load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, const OBJ& obj,
                                                Loads& o)
    {
        const int64_t rc = obj.rows * obj.cols;
        volume_load(v, vi, nv, n, rc, obj.cols, rc % W == 0, obj.cols % W == 0, o);
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
#pragma unroll
        for (int s = 0; s < 3; s++)
#pragma unroll
            for (int r = 0; r < 3; r++)
            {
#pragma unroll
                for (int k = 0; k < W; k++)
                    x.p[s][r].e[k] = xp.p[s][r].e[k] + step * d.p[s][r].e[k];
                x.edge[s][r][0] = xp.edge[s][r][0] + step * d.edge[s][r][0];
            }
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l) { return l.p[1][1]; }
    // the nine windows of the pack at vi from the values a lane holds; called by all 64 lanes of the wave
    template <class LD, class BODY>
    __device__ __forceinline__ static void gather(const Loads& xv, int64_t vi, int64_t nv, int64_t n, const OBJ& obj, LD ld,
                                                  BODY body)
    {
        const int64_t cols = obj.cols, rc = obj.rows * cols, b = vi * W;
        auto right = [&](int64_t e) { return (e >= 0 && e < n) ? ld(e) : T(0); };
        Win w00, w01, w02, w10, w11, w12, w20, w21, w22;
#define LBFGSX_VOLUME_WINDOW(S, R, WIN) \
    chain_window<T, 2>(xv.p[S][R], xv.edge[S][R], vi, nv, [&](int j) { return right(b + (S - 1) * rc + (R - 1) * cols + W + j); }, WIN)
        LBFGSX_VOLUME_WINDOW(0, 0, w00);
        LBFGSX_VOLUME_WINDOW(0, 1, w01);
        LBFGSX_VOLUME_WINDOW(0, 2, w02);
        LBFGSX_VOLUME_WINDOW(1, 0, w10);
        LBFGSX_VOLUME_WINDOW(1, 1, w11);
        LBFGSX_VOLUME_WINDOW(1, 2, w12);
        LBFGSX_VOLUME_WINDOW(2, 0, w20);
        LBFGSX_VOLUME_WINDOW(2, 1, w21);
        LBFGSX_VOLUME_WINDOW(2, 2, w22);
#undef LBFGSX_VOLUME_WINDOW
        body(w00, w01, w02, w10, w11, w12, w20, w21, w22);
    }
    // the gradient of the pack at vi (position pos) from its nine windows, and the values of the cells that start inside it:
    // the four passes in ascending cell origin, which is the order of the adds into a coordinate
    template <class A>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T>& g, A& fx,
                                                const Win& w00, const Win& w01, const Win& w02, const Win& w10, const Win& w11,
                                                const Win& w12, const Win& w20, const Win& w21, const Win& w22)
    {
        const int64_t b = vi * W;
        bool has[W];
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            has[k] = false;
            g.e[k] = T(0);
        }
        if (pos.slab >= 1 && pos.slab + 1 < obj.slabs && pos.row >= 1 && pos.row + 1 < obj.rows && pos.col >= 1 &&
            pos.col + W + 1 <= obj.cols)
        {
            volume_cell_row<true, 0, 0>(obj, b, pos, w00, w01, w10, w11, g, has, fx);
            volume_cell_row<true, 0, 1>(obj, b, pos, w01, w02, w11, w12, g, has, fx);
            volume_cell_row<true, 1, 0>(obj, b, pos, w10, w11, w20, w21, g, has, fx);
            volume_cell_row<true, 1, 1>(obj, b, pos, w11, w12, w21, w22, g, has, fx);
        }
        else
        {
            volume_cell_row<false, 0, 0>(obj, b, pos, w00, w01, w10, w11, g, has, fx);
            volume_cell_row<false, 0, 1>(obj, b, pos, w01, w02, w11, w12, g, has, fx);
            volume_cell_row<false, 1, 0>(obj, b, pos, w10, w11, w20, w21, g, has, fx);
            volume_cell_row<false, 1, 1>(obj, b, pos, w11, w12, w21, w22, g, has, fx);
        }
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        return volume_tail<T>(obj, i, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_volume, halo_eval, halo_trial, VolumeFamily<T, OBJ>)

}  // namespace lbfgsx
