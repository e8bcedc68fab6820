// lbfgspp_amd/csrc/halo_frame.cuh -- the frame of the halo kernels: the four evaluation kernels of a CHAIN, of a GRID and of
// a VOLUME objective (chain_kernels.cuh, grid_kernels.cuh, volume_kernels.cuh) are halo_eval and halo_trial, bounded or not,
// around the family's loads, windows and terms.  Their parameter lists, BOUNDED conventions, outputs, tile order, reductions and completion signal are
// those of own_eval / own_trial (own_frame.cuh), that is of k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial.
//
// Ownership.  A thread owns the W = 16 / sizeof(T) coordinates of a 16-byte pack: it writes their grad (and x in the trial
// kernels) and adds the terms that start there to f.  A term reads coordinates of neighbouring packs, the halo.  Adjacent
// lanes hold adjacent packs and hand each other their halo by cross-lane moves, so every loop below runs from the WAVE's
// first pack with all 64 lanes in it, whether a lane holds a pack (vi < nv) or not; only a lane without a neighbour loads
// its halo, with its pack.  Thread 0 of block 0 also owns the coordinates past the last whole pack, one at a time.
//
// A family F supplies what differs:
//     static constexpr int U                               the tile depth of the two trial kernels
//     struct Loads                                         what a lane holds of ONE vector for pack vi: packs and the halo
//                                                          it has no neighbour for
//     void load(v, vi, nv, n, obj, Loads&)                 ... loaded from v: zero where the lane holds no pack or the
//                                                          coordinate is outside [0, n)
//     void axpy(xp, d, step, Loads& x)                     x = xp + step*d on everything a lane holds
//     const Pack<T>& own(const Loads&)                     the lane's own pack
//     void gather(Loads, vi, nv, n, obj, ld, body)         puts the windows of pack vi together from the wave's Loads, in
//                                                          arrays of its own, and calls body(windows...) once: called by
//                                                          all 64 lanes; ld(i) = x[i] from memory (x itself in the
//                                                          evaluation kernels, xp[i] + step*d[i] in the trial kernels --
//                                                          never a read of the x the launch writes), for 0 <= i < n only
//     struct Pos;  Pos pos(obj, flat);  void advance(obj, Pos&, step);  void retreat(obj, Pos&, step)
//                                                          what a family carries along the loop about a pack's position
//                                                          (the grid's row and column, the volume's slab too; nothing for a
//                                                          chain)
//     void pack(obj, vi, n, pos, Pack<T>& g, A& fx, windows...)   pack vi: its W partial derivatives, the terms it owns to fx
//     T tail(obj, i, n, ld, fx)                            coordinate i past the last whole pack: the same
// The windows are the family's own arrays and reach pack through the frame's body, not as one object the frame holds: as one
// object (a struct of the grid's three windows, or an array of them) k_grid_trial in f32 compiles to 142 VGPRs and 3 waves
// per SIMD, as three arrays to the 4 waves it had (profiles/own_frame_kernel_resources.tsv).
#pragma once
#include "lbfgs_kernels.cuh"
#include "lbfgsb_kernels.cuh"
#include "frame_kernels.cuh"

namespace lbfgsx {

// ---------------------------------------------------------------- k_eval's and k_b_eval's counterparts
// BOUNDED false: out[0] = f(x), out[1] = g.g, out[2] = x.x;  true: out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class F, class OBJ, bool BOUNDED>
__device__ __forceinline__ void halo_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                          const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    constexpr int NA = BOUNDED ? 2 : 3, XX = NA - 1;  // acc[0]: f's sum, acc[XX]: x.x, acc[1] of three: g.g
    A acc[NA];
    double pgm = 0.0;
    const int64_t nv = n / W;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    auto ld = [&](int64_t i) { return x[i]; };
    const typename F::Pos step = F::pos(obj, stride * W);
    typename F::Pos pos = F::pos(obj, (int64_t(blockIdx.x) * kBlock + threadIdx.x) * W);
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        typename F::Loads xv;
        Pack<T> pl, pu;
        F::load(x, vi, nv, n, obj, xv);
        if constexpr (BOUNDED)
            if (vi < nv)
            {
                pl = ldv(lb, vi);
                pu = ldv(ub, vi);
            }
        F::gather(xv, vi, nv, n, obj, ld, [&](const auto&... win) __attribute__((always_inline)) {
            if (vi >= nv)
                return;
            const Pack<T>& px = F::own(xv);
            Pack<T> pg;
            F::pack(obj, vi, n, pos, pg, acc[0], win...);
            stv(g, vi, pg);
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                acc[XX].add_prod(px.e[k], px.e[k]);
                if constexpr (BOUNDED)
                    pgm = fmax(pgm, double(projg_term(px.e[k], pg.e[k], pl.e[k], pu.e[k])));
                else
                    acc[1].add_prod(pg.e[k], pg.e[k]);
            }
        });
        F::advance(obj, pos, step);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = F::tail(obj, i, n, ld, acc[0]);
            g[i] = gi;
            acc[XX].add_prod(x[i], x[i]);
            if constexpr (BOUNDED)
                pgm = fmax(pgm, double(projg_term(x[i], gi, lb[i], ub[i])));
            else
                acc[1].add_prod(gi, gi);
        }
    if constexpr (BOUNDED)
        ext_publish<false>(pgm, ws, 4);
    if (grid_reduce<NA>(acc, ws))
    {
        double pgmax = 0.0;
        if constexpr (BOUNDED)
            pgmax = ext_collect<false>(ws, 4);
        if (threadIdx.x == 0)
        {
            out[0] = T(acc[0].value());
            out[1] = T(acc[1].value());
            out[2] = BOUNDED ? T(pgmax) : T(acc[XX].value());
        }
    }
}

// ---------------------------------------------------------------- k_trial's and k_b_dg_maxstep_trial's counterparts
// x = xp + step*d ; g = grad f(x).  BOUNDED false: out[0] = f(x), out[1] = g.d;
// true: out[0] = g0.d, out[1] = step_max, out[2] = f(x), out[3] = grad(x).d
template <class T, class F, class OBJ, bool BOUNDED>
__device__ __forceinline__ void halo_trial(const T* __restrict__ xp, const T* __restrict__ g0, const T* __restrict__ d,
                                           const T* __restrict__ lb, const T* __restrict__ ub, T step, T* __restrict__ x,
                                           T* __restrict__ g, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, U = F::U;
    constexpr int NA = BOUNDED ? 3 : 2;
    A acc[NA];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t nv = n / W;
    const int64_t tile = int64_t(kBlock) * U;
    const int64_t top = ((nv + tile - 1) / tile - 1) * tile;
    auto ld = [&](int64_t i) { return xp[i] + step * d[i]; };
    const typename F::Pos ustep = F::pos(obj, int64_t(kBlock) * W);
    const typename F::Pos tstep = F::pos(obj, int64_t(gridDim.x) * tile * W);
    const int64_t first = int64_t(blockIdx.x) * tile;
    typename F::Pos pos0 = {};
    if (first < nv)
        pos0 = F::pos(obj, ((rev ? top - first : first) + threadIdx.x) * W);
    for (int64_t t0 = first; t0 < nv; t0 += int64_t(gridDim.x) * tile)  // the block's: all lanes stay in
    {
        const int64_t base = (rev ? top - t0 : t0) + threadIdx.x;
        typename F::Loads lxp[U], ldd[U];
        Pack<T> pg0[U], plo[U], pup[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            F::load(xp, vi, nv, n, obj, lxp[u]);
            F::load(d, vi, nv, n, obj, ldd[u]);
            if constexpr (BOUNDED)
                if (vi < nv)
                {
                    pg0[u] = ldv<T>(g0, vi);
                    plo[u] = ldv<T>(lb, vi);
                    pup[u] = ldv<T>(ub, vi);
                }
        }
        typename F::Pos pos = pos0;
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            typename F::Loads xv;
            F::axpy(lxp[u], ldd[u], step, xv);
            F::gather(xv, vi, nv, n, obj, ld, [&](const auto&... win) __attribute__((always_inline)) {
                if (vi >= nv)
                    return;
                const Pack<T>& pxp = F::own(lxp[u]);
                const Pack<T>& pd = F::own(ldd[u]);
                Pack<T> pg;
                if constexpr (BOUNDED)
                {
#pragma unroll
                    for (int k = 0; k < W; k++)
                    {
                        if constexpr (U == 1)
                        {
                            // the bounds by value, read first: as operands of feas the two reads are sunk into the branches on
                            // d's sign and, at this depth (k_volume_b_dg_maxstep_trial), lb's and ub's packs then live in 48
                            // bytes of scratch.  The deeper tiles keep the statements they were measured with
                            const T lo = plo[u].e[k], up = pup[u].e[k];
                            acc[NA - 1].add_prod(pg0[u].e[k], pd.e[k]);
                            feas(pxp.e[k], pd.e[k], lo, up);
                        }
                        else
                        {
                            acc[NA - 1].add_prod(pg0[u].e[k], pd.e[k]);
                            feas(pxp.e[k], pd.e[k], plo[u].e[k], pup[u].e[k]);
                        }
                    }
                }
                F::pack(obj, vi, n, pos, pg, acc[0], win...);
                stv<T>(x, vi, F::own(xv));
                stv<T>(g, vi, pg);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[1].add_prod(pg.e[k], pd.e[k]);
            });
            F::advance(obj, pos, ustep);
        }
        if (rev)
            F::retreat(obj, pos0, tstep);
        else
            F::advance(obj, pos0, tstep);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            if constexpr (BOUNDED)
            {
                acc[NA - 1].add_prod(g0[i], d[i]);
                feas(xp[i], d[i], lb[i], ub[i]);
            }
            x[i] = xp[i] + step * d[i];
            const T gi = F::tail(obj, i, n, ld, acc[0]);
            g[i] = gi;
            acc[1].add_prod(gi, d[i]);
        }
    if constexpr (BOUNDED)
        ext_publish<true>(smin, ws, 6);
    if (grid_reduce<NA>(acc, ws))
    {
        double smin_all = 0.0;
        if constexpr (BOUNDED)
            smin_all = ext_collect<true>(ws, 6);
        if (threadIdx.x == 0)
        {
            if constexpr (BOUNDED)
            {
                out[0] = T(acc[2].value());
                out[1] = T(smin_all);
            }
            out[BOUNDED ? 2 : 0] = T(acc[0].value());
            out[BOUNDED ? 3 : 1] = T(acc[1].value());
            ws_signal(ws);
        }
    }
}

}  // namespace lbfgsx
