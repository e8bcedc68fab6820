// lbfgspp_amd/csrc/periodic_volume_kernels.cuh -- the four evaluation kernels for a PERIODIC VOLUME objective
//     f(x) = sum over the cells (s, r, c) that exist of phi(x[8]; s, r, c),   x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc],
//     + modulo the extent,
// on a slab-major slabs x rows x cols array x, n = slabs*rows*cols; cell (s, r, c) exists iff (c < cols-1 or bit 0 of
// obj.periodic) and (r < rows-1 or bit 1) and (s < slabs-1 or bit 2) (include/lbfgsx.h, "periodic grid and volume
// objectives").  With the mask 0 this is the volume objective of volume_kernels.cuh.
//
// k_pvolume_eval, k_pvolume_trial, k_pvolume_b_eval and k_pvolume_b_dg_maxstep_trial take the arguments of k_eval, k_trial,
// k_b_eval and k_b_dg_maxstep_trial and are launched with their grids.  They are halo_eval and halo_trial (halo_frame.cuh)
// around PeriodicVolumeFamily, which is to VolumeFamily what PeriodicGridFamily (periodic_grid_kernels.cuh) is to GridFamily.
// Compiled at run time only (jit_objective.hip): OBJ is the struct generated around the caller's text for one cell,
//     int64_t slabs, rows, cols;  int periodic;
//     T term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col, const int64_t (&j)[8]) const;
// j: the flat indices of the cell's eight corners, j[0] == i.
//
// Ownership and order are the volume form's: grad of (s, r, c) is the sum of g[7] of cell (s-1, r-1, c-1), g[6] of
// (s-1, r-1, c), g[5] of (s-1, r, c-1), g[4] of (s-1, r, c), g[3] of (s, r-1, c-1), g[2] of (s, r-1, c), g[1] of (s, r, c-1) and
// g[0] of (s, r, c) -- those that exist, in this order, started from the first, - modulo the extent on a periodic axis.
//
// The nine windows are the volume form's, by the same cross-lane moves with all 64 lanes in them.  What differs:
//   the slab direction  wraps uniformly in the flat index, +- rows*cols mod n, in the loads (pvolume_load): aligned 16-byte
//       loads of the wrapped packs under the volume form's alignment conditions (rows*cols % W == 0 makes n % W == 0), element
//       loads of the wrapped coordinates otherwise.  Where it is open they load what volume_load loads.
//   the column direction  as in the periodic grid: a pack that lies inside one row keeps its windows and its 4(W+1) cells;
//       in column 0 the nine left-hand halo values, at column cols-1 the nine right-hand ones are element loads by the
//       frame's ld.
//   the row direction  a pack in row 0 takes the three windows one row above, a pack in row rows-1 the three one row below,
//       from the other end of the same slab: 3(W+2) element loads by ld.  That is one pair of rows per slab.
//   A patch loads only into windows that a pass which exists reads (not the slab above a pack of slab 0 on an open axis).
//   a pack that straddles the end of a row  (only when cols % W != 0) goes coordinate by coordinate through the tail's function.
// Every pack inside a row runs the same cells, so a wave with seam packs in it runs nothing twice.  No index outside [0, n) is
// loaded.
#pragma once
#include "periodic_grid_kernels.cuh"
#include "volume_kernels.cuh"

namespace lbfgsx {

// volume_load with everything wrapped modulo n when wrap is set (the slab direction); with it clear, volume_load's loads
template <class T>
__device__ __forceinline__ void pvolume_load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, int64_t rc, int64_t cols,
                                             bool slab_aligned, bool row_aligned, bool wrap, VolumeLoads<T>& o)
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
                else if (aligned && (wrap ? slab_aligned : (lo >= 0 && lo + W <= n)))  // wrapped: n must be a multiple of W too
                    o.p[s][r] = ldv(v, wrap_once(lo, n) / W);
                else
                {
#pragma unroll
                    for (int k = 0; k < W; k++)
                    {
                        const int64_t w = wrap_once(lo + k, n);
                        if (wrap || w == lo + k)
                            o.p[s][r].e[k] = v[w];
                    }
                }
                if (lane == 0 || lane == 63 || vi + 1 >= nv)
                {
                    const int64_t e = (lane == 0) ? lo - 1 : lo + W;
                    const int64_t w = wrap_once(e, n);
                    if (wrap || w == e)
                        o.edge[s][r][0] = v[w];
                }
            }
        }
}

// coordinate i on its own (one past the last whole pack, or one of a pack that straddles the end of a row): its up to eight
// cells with every corner from ld(k) = x[k], 0 <= k < n; its partial derivative, returned, and the value of the cell that
// starts there, added to fx
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T pvolume_node(const OBJ& obj, int64_t i, LD ld, A& fx)
{
    const int64_t cols = obj.cols, rows = obj.rows, slabs = obj.slabs;
    const int per = obj.periodic;
    const VolumePos p = volume_pos(i, rows, cols);
    T gi = T(0);
    bool has = false;
#pragma unroll 1
    for (int q = 0; q < 8; q++)  // cells (s-1, r-1, c-1) .. (s, r, c): ascending origin; i is their corner 7 - q
    {
        // per axis: the cell starts at the coordinate (the bit of q set) or one before it, modulo the extent
        const bool os = (q & 4) != 0, orow = (q & 2) != 0, oc = (q & 1) != 0;
        const bool ex = ((per & 4) || (os ? p.slab + 1 < slabs : p.slab > 0)) && ((per & 2) || (orow ? p.row + 1 < rows : p.row > 0)) &&
                        ((per & 1) || (oc ? p.col + 1 < cols : p.col > 0));
        if (ex)
        {
            const int64_t s0 = os ? p.slab : (p.slab > 0 ? p.slab - 1 : slabs - 1), s1 = s0 + 1 < slabs ? s0 + 1 : 0;
            const int64_t r0 = orow ? p.row : (p.row > 0 ? p.row - 1 : rows - 1), r1 = r0 + 1 < rows ? r0 + 1 : 0;
            const int64_t c0 = oc ? p.col : (p.col > 0 ? p.col - 1 : cols - 1), c1 = c0 + 1 < cols ? c0 + 1 : 0;
            const int64_t b00 = (s0 * rows + r0) * cols, b01 = (s0 * rows + r1) * cols, b10 = (s1 * rows + r0) * cols,
                          b11 = (s1 * rows + r1) * cols;
            const int64_t tj[8] = {b00 + c0, b00 + c1, b01 + c0, b01 + c1, b10 + c0, b10 + c1, b11 + c0, b11 + c1};
            const T tx[8] = {ld(tj[0]), ld(tj[1]), ld(tj[2]), ld(tj[3]), ld(tj[4]), ld(tj[5]), ld(tj[6]), ld(tj[7])};
            T tg[8];
            const T v = obj.term(tx, tg, tj[0], s0, r0, c0, tj);
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

// the cells whose origins are the first W+1 positions of the window w00, for a pack at column col that lies inside one row:
// PS 0 the slab above the pack, 1 its own; PR 0 the row above, 1 its own.  The pack's coordinates are the cells' corners
// 4*(1-PS) + 2*(1-PR) + dc.  w<ds><dr>: the windows of the cells' slab (ds 0) and the one below, of the cells' row (dr 0) and the
// one below; (s0, r0): the cells' slab and row; b<ds><dr>: the flat index of column 0 of the four rows
template <int PS, int PR, class T, class OBJ, class A>
__device__ __forceinline__ void pvolume_cell_row(const OBJ& obj, int64_t col, int64_t s0, int64_t r0, int64_t b00, int64_t b01,
                                                 int64_t b10, int64_t b11, const T (&w00)[Vec16<T>::W + 2],
                                                 const T (&w01)[Vec16<T>::W + 2], const T (&w10)[Vec16<T>::W + 2],
                                                 const T (&w11)[Vec16<T>::W + 2], Pack<T>& g, bool (&has)[Vec16<T>::W], A& fx)
{
    constexpr int W = Vec16<T>::W;
    constexpr int jl = 4 * (1 - PS) + 2 * (1 - PR), jr = jl + 1;
    const int64_t cols = obj.cols;
    const bool pc = (obj.periodic & 1) != 0;
#pragma unroll
    for (int s = 0; s <= W; s++)
    {
        if ((s == 0 && !(col > 0 || pc)) || (s == W && !(col + W < cols || pc)))
            continue;
        const int64_t c0 = (s == 0 && col == 0) ? cols - 1 : col - 1 + s;
        const int64_t c1 = (s == W && col + W == cols) ? 0 : col + s;
        const T tx[8] = {w00[s], w00[s + 1], w01[s], w01[s + 1], w10[s], w10[s + 1], w11[s], w11[s + 1]};
        const int64_t tj[8] = {b00 + c0, b00 + c1, b01 + c0, b01 + c1, b10 + c0, b10 + c1, b11 + c0, b11 + c1};
        T tg[8];
        const T v = obj.term(tx, tg, tj[0], s0, r0, c0, tj);
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
}

// the frame's family (halo_frame.cuh): VolumeFamily's loads with the slab direction wrapped, its windows with the frame's ld
// behind them, and a pack that patches the row and the column seams
template <class T, class OBJ>
struct PeriodicVolumeFamily
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
        pvolume_load(v, vi, nv, n, rc, obj.cols, rc % W == 0, obj.cols % W == 0, (obj.periodic & 4) != 0, o);
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
        VolumeFamily<T, OBJ>::axpy(xp, d, step, x);
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l) { return l.p[1][1]; }
    template <class LD, class BODY>
    __device__ __forceinline__ static void gather(const Loads& xv, int64_t vi, int64_t nv, int64_t n, const OBJ& obj, LD ld,
                                                  BODY body)
    {
        const int64_t cols = obj.cols, rc = obj.rows * cols, b = vi * W;
        const bool wrap = (obj.periodic & 4) != 0;
        auto right = [&](int64_t e) {
            const int64_t w = wrap_once(e, n);
            return (wrap || w == e) ? ld(w) : T(0);
        };
        Win w00, w01, w02, w10, w11, w12, w20, w21, w22;
#define LBFGSX_PVOLUME_WINDOW(S, R, WIN) \
    chain_window<T, 2>(xv.p[S][R], xv.edge[S][R], vi, nv, [&](int j) { return right(b + (S - 1) * rc + (R - 1) * cols + W + j); }, WIN)
        LBFGSX_PVOLUME_WINDOW(0, 0, w00);
        LBFGSX_PVOLUME_WINDOW(0, 1, w01);
        LBFGSX_PVOLUME_WINDOW(0, 2, w02);
        LBFGSX_PVOLUME_WINDOW(1, 0, w10);
        LBFGSX_PVOLUME_WINDOW(1, 1, w11);
        LBFGSX_PVOLUME_WINDOW(1, 2, w12);
        LBFGSX_PVOLUME_WINDOW(2, 0, w20);
        LBFGSX_PVOLUME_WINDOW(2, 1, w21);
        LBFGSX_PVOLUME_WINDOW(2, 2, w22);
#undef LBFGSX_PVOLUME_WINDOW
        body(w00, w01, w02, w10, w11, w12, w20, w21, w22, ld);
    }
    template <class A, class LD>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t, const Pos& pos, Pack<T>& g, A& fx,
                                                const Win& w00, const Win& w01, const Win& w02, const Win& w10, const Win& w11,
                                                const Win& w12, const Win& w20, const Win& w21, const Win& w22, const LD& ld)
    {
        const int64_t cols = obj.cols, rows = obj.rows, slabs = obj.slabs, slab = pos.slab, row = pos.row, col = pos.col;
#pragma unroll
        for (int k = 0; k < W; k++)
            g.e[k] = T(0);
        if (col + W > cols)  // the pack straddles the end of a row
        {
#pragma unroll 1
            for (int k = 0; k < W; k++)
            {
                const T gi = pvolume_node<T>(obj, vi * W + k, ld, fx);
#pragma unroll
                for (int kk = 0; kk < W; kk++)
                    g.e[kk] = (kk == k) ? gi : g.e[kk];
            }
            return;
        }
        const bool pc = (obj.periodic & 1) != 0, pr = (obj.periodic & 2) != 0, ps = (obj.periodic & 4) != 0;
        const int64_t ss[3] = {slab > 0 ? slab - 1 : slabs - 1, slab, slab + 1 < slabs ? slab + 1 : 0};
        const int64_t rr[3] = {row > 0 ? row - 1 : rows - 1, row, row + 1 < rows ? row + 1 : 0};
        // the flat index of column 0 of the nine rows, formed where it is used
        auto base_of = [&](int ds, int dr) { return (ss[ds] * rows + rr[dr]) * cols; };
        T w[3][3][W + 2];
#pragma unroll
        for (int s = 0; s < W + 2; s++)
        {
            w[0][0][s] = w00[s];
            w[0][1][s] = w01[s];
            w[0][2][s] = w02[s];
            w[1][0][s] = w10[s];
            w[1][1][s] = w11[s];
            w[1][2][s] = w12[s];
            w[2][0][s] = w20[s];
            w[2][1][s] = w21[s];
            w[2][2][s] = w22[s];
        }
        const int64_t cl = col > 0 ? col - 1 : cols - 1, cr = col + W < cols ? col + W : 0;  // the columns of the two halo values
        const bool hs[2] = {slab > 0 || ps, slab + 1 < slabs || ps}, hr[2] = {row > 0 || pr, row + 1 < rows || pr};
        const bool us[3] = {hs[0], true, hs[1]}, ur[3] = {hr[0], true, hr[1]};  // does a pass that exists read window [ds][dr]
        if (pr && (row == 0 || row + 1 == rows))  // the row beyond the seam is the slab's other end
        {
            const bool top = row == 0;  // rows >= 2: never both
#pragma unroll
            for (int ds = 0; ds < 3; ds++)
            {
                if (!us[ds])
                    continue;
                const int64_t bs = top ? base_of(ds, 0) : base_of(ds, 2);
#pragma unroll
                for (int s = 0; s < W + 2; s++)
                {
                    const T val = ld(bs + (s == 0 ? cl : (s == W + 1 ? cr : col - 1 + s)));
                    if (top)
                        w[ds][0][s] = val;
                    else
                        w[ds][2][s] = val;
                }
            }
        }
        if (pc && col == 0)  // the nodes to the left of column 0 are the row's last
        {
#pragma unroll
            for (int ds = 0; ds < 3; ds++)
#pragma unroll
                for (int dr = 0; dr < 3; dr++)
                    if (us[ds] && ur[dr])
                        w[ds][dr][0] = ld(base_of(ds, dr) + cols - 1);
        }
        if (pc && col + W == cols)  // the nodes to the right of column cols-1 are the row's first
        {
#pragma unroll
            for (int ds = 0; ds < 3; ds++)
#pragma unroll
                for (int dr = 0; dr < 3; dr++)
                    if (us[ds] && ur[dr])
                        w[ds][dr][W + 1] = ld(base_of(ds, dr));
        }
        bool has[W];
#pragma unroll
        for (int k = 0; k < W; k++)
            has[k] = false;
#define LBFGSX_PVOLUME_PASS(PS, PR)                                                                                             \
    if (hs[PS] && hr[PR])                                                                                                       \
    pvolume_cell_row<PS, PR>(obj, col, ss[PS], rr[PR], base_of(PS, PR), base_of(PS, PR + 1), base_of(PS + 1, PR), base_of(PS + 1, PR + 1),     \
                             w[PS][PR], w[PS][PR + 1], w[PS + 1][PR], w[PS + 1][PR + 1], g, has, fx)
        LBFGSX_PVOLUME_PASS(0, 0);
        LBFGSX_PVOLUME_PASS(0, 1);
        LBFGSX_PVOLUME_PASS(1, 0);
        LBFGSX_PVOLUME_PASS(1, 1);
#undef LBFGSX_PVOLUME_PASS
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t, LD ld, A& fx)
    {
        return pvolume_node<T>(obj, i, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_pvolume, halo_eval, halo_trial, PeriodicVolumeFamily<T, OBJ>)

}  // namespace lbfgsx
