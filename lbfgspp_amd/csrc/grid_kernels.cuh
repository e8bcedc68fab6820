// lbfgspp_amd/csrc/grid_kernels.cuh -- the four evaluation kernels for a GRID objective
//     f(x) = sum over cells (r, c), 0 <= r < rows-1, 0 <= c < cols-1, of phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c)
// on a row-major rows x cols array x, n = rows*cols (include/lbfgsx.h, "grid objectives").
//
// k_grid_eval, k_grid_trial, k_grid_b_eval and k_grid_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval and
// k_b_dg_maxstep_trial and are launched with their grids: the same outputs, tile order, reductions and completion signal;
// launch_args.hpp serves all three families.  They are compiled at run time only (jit_objective.hip): OBJ is the struct
// generated around the caller's text for one cell,
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

// ---------------------------------------------------------------- k_eval's counterpart
// out[0] = f(x), out[1] = g.g, out[2] = x.x
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_grid_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                      T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[3];
    const int64_t cols = obj.cols;
    const bool aligned = cols % W == 0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    const GridPos step = grid_pos(stride * W, cols);
    GridPos pos = grid_pos((int64_t(blockIdx.x) * kBlock + threadIdx.x) * W, cols);
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        GridLoads<T> xv;
        T up[W + 2], mid[W + 2], dn[W + 2];
        grid_load(x, vi, nv, n, cols, aligned, xv);
        grid_windows(xv, vi, nv, n, cols, [&](int64_t e) { return x[e]; }, up, mid, dn);
        if (vi < nv)
        {
            Pack<T> pg;
            grid_pack(obj, vi, pos, up, mid, dn, pg, acc[0]);
            stv(g, vi, pg);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[1].add_prod(pg.e[k], pg.e[k]);
                acc[2].add_prod(xv.p[1].e[k], xv.p[1].e[k]);
            }
        }
        grid_advance(pos, step, cols);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = grid_tail<T>(obj, i, [&](int64_t k) { return x[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, gi);
            acc[2].add_prod(x[i], x[i]);
        }
    if (grid_reduce<3>(acc, ws) && threadIdx.x == 0)
    {
        out[0] = T(acc[0].value());
        out[1] = T(acc[1].value());
        out[2] = T(acc[2].value());
    }
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

// ---------------------------------------------------------------- k_trial's counterpart
// x = xp + step*d ; g = grad f(x) ; out[0] = f(x), out[1] = g.d
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_grid_trial(const T* __restrict__ xp, const T* __restrict__ d, T step,
                                                       T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                       T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kGridTrialU;
    A acc[2];
    const int64_t cols = obj.cols;
    const bool aligned = cols % W == 0;
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    const GridPos ustep = grid_pos(int64_t(kBlock) * W, cols);
    const GridPos tstep = grid_pos(int64_t(gridDim.x) * tile * W, cols);
    const int64_t first = int64_t(blockIdx.x) * tile;
    GridPos pos0 = {0, 0};
    if (first < nv)
        pos0 = grid_pos(((rev ? top - first : first) + threadIdx.x) * W, cols);
    for (int64_t t0 = first; t0 < nv; t0 += int64_t(gridDim.x) * tile)  // the block's: all lanes stay in
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        GridLoads<T> lxp[U], ld_[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            grid_load(xp, base + u * kBlock, nv, n, cols, aligned, lxp[u]);
            grid_load(d, base + u * kBlock, nv, n, cols, aligned, ld_[u]);
        }
        GridPos pos = pos0;
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            GridLoads<T> xv;
            T up[W + 2], mid[W + 2], dn[W + 2];
            grid_axpy(lxp[u], ld_[u], step, xv);
            grid_windows(xv, vi, nv, n, cols, [&](int64_t e) { return xp[e] + step * d[e]; }, up, mid, dn);
            if (vi < nv)
            {
                Pack<T> pg;
                grid_pack(obj, vi, pos, up, mid, dn, pg, acc[0]);
                stv(x, vi, xv.p[1]);
                stv(g, vi, pg);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[1].add_prod(pg.e[k], ld_[u].p[1].e[k]);
            }
            grid_advance(pos, ustep, cols);
        }
        if (rev)
            grid_retreat(pos0, tstep, cols);
        else
            grid_advance(pos0, tstep, cols);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            x[i] = xp[i] + step * d[i];
            const T gi = grid_tail<T>(obj, i, [&](int64_t k) { return xp[k] + step * d[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
    if (grid_reduce<2>(acc, ws) && threadIdx.x == 0)
    {
        out[0] = T(acc[0].value());
        out[1] = T(acc[1].value());
        ws_signal(ws);
    }
}

// ---------------------------------------------------------------- k_b_eval's counterpart
// out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_grid_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                        const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws,
                                                        T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    A acc[2];
    double pg = 0.0;
    const int64_t cols = obj.cols;
    const bool aligned = cols % W == 0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    const GridPos step = grid_pos(stride * W, cols);
    GridPos pos = grid_pos((int64_t(blockIdx.x) * kBlock + threadIdx.x) * W, cols);
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        GridLoads<T> xv;
        Pack<T> pl, pu;
        T up[W + 2], mid[W + 2], dn[W + 2];
        grid_load(x, vi, nv, n, cols, aligned, xv);
        if (vi < nv)
        {
            pl = ldv(lb, vi);
            pu = ldv(ub, vi);
        }
        grid_windows(xv, vi, nv, n, cols, [&](int64_t e) { return x[e]; }, up, mid, dn);
        if (vi < nv)
        {
            Pack<T> pgv;
            grid_pack(obj, vi, pos, up, mid, dn, pgv, acc[0]);
            stv(g, vi, pgv);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[1].add_prod(xv.p[1].e[k], xv.p[1].e[k]);
                pg = fmax(pg, double(projg_term(xv.p[1].e[k], pgv.e[k], pl.e[k], pu.e[k])));
            }
        }
        grid_advance(pos, step, cols);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = grid_tail<T>(obj, i, [&](int64_t k) { return x[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(x[i], x[i]);
            pg = fmax(pg, double(projg_term(x[i], gi, lb[i], ub[i])));
        }
    ext_publish<false>(pg, ws, 4);
    if (grid_reduce<2>(acc, ws))
    {
        const double pgmax = ext_collect<false>(ws, 4);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[0].value());
            out[1] = T(acc[1].value());
            out[2] = T(pgmax);
        }
    }
}

// ---------------------------------------------------------------- k_b_dg_maxstep_trial's counterpart
// out[0] = g0.d, out[1] = step_max, out[2] = f(x), out[3] = grad(x).d at x = xp + step*d
template <class T, class OBJ>
__global__ void __launch_bounds__(kBlock) k_grid_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0,
                                                                    const T* __restrict__ d, const T* __restrict__ lb,
                                                                    const T* __restrict__ ub, T step, T* __restrict__ x,
                                                                    T* __restrict__ g, int64_t n, OBJ obj, RedWs ws,
                                                                    T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int U = kGridTrialU;
    A acc[3];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t cols = obj.cols;
    const bool aligned = cols % W == 0;
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    const GridPos ustep = grid_pos(int64_t(kBlock) * W, cols);
    const GridPos tstep = grid_pos(int64_t(gridDim.x) * tile * W, cols);
    const int64_t first = int64_t(blockIdx.x) * tile;
    GridPos pos0 = {0, 0};
    if (first < nv)
        pos0 = grid_pos(((rev ? top - first : first) + threadIdx.x) * W, cols);
    for (int64_t t0 = first; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        GridLoads<T> lxp[U], ld_[U];
        Pack<T> pg0[U], plo[U], pup[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            grid_load(xp, vi, nv, n, cols, aligned, lxp[u]);
            grid_load(d, vi, nv, n, cols, aligned, ld_[u]);
            if (vi < nv)
            {
                pg0[u] = ldv<T>(g0, vi);
                plo[u] = ldv<T>(lb, vi);
                pup[u] = ldv<T>(ub, vi);
            }
        }
        GridPos pos = pos0;
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            GridLoads<T> xv;
            T up[W + 2], mid[W + 2], dn[W + 2];
            grid_axpy(lxp[u], ld_[u], step, xv);
            grid_windows(xv, vi, nv, n, cols, [&](int64_t e) { return xp[e] + step * d[e]; }, up, mid, dn);
            if (vi < nv)
            {
                Pack<T> pg;
#pragma unroll
                for (int k = 0; k < W; k++)
                {
                    acc[2].add_prod(pg0[u].e[k], ld_[u].p[1].e[k]);
                    feas(lxp[u].p[1].e[k], ld_[u].p[1].e[k], plo[u].e[k], pup[u].e[k]);
                }
                grid_pack(obj, vi, pos, up, mid, dn, pg, acc[0]);
                stv<T>(x, vi, xv.p[1]);
                stv<T>(g, vi, pg);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[1].add_prod(pg.e[k], ld_[u].p[1].e[k]);
            }
            grid_advance(pos, ustep, cols);
        }
        if (rev)
            grid_retreat(pos0, tstep, cols);
        else
            grid_advance(pos0, tstep, cols);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            acc[2].add_prod(g0[i], d[i]);
            feas(xp[i], d[i], lb[i], ub[i]);
            x[i] = xp[i] + step * d[i];
            const T gi = grid_tail<T>(obj, i, [&](int64_t k) { return xp[k] + step * d[k]; }, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
    ext_publish<true>(smin, ws, 6);
    if (grid_reduce<3>(acc, ws))
    {
        const double smin_all = ext_collect<true>(ws, 6);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[2].value());
            out[1] = T(smin_all);
            out[2] = T(acc[0].value());
            out[3] = T(acc[1].value());
            ws_signal(ws);
        }
    }
}

}  // namespace lbfgsx
