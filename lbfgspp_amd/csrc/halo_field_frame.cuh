// lbfgspp_amd/csrc/halo_field_frame.cuh -- halo_frame.cuh for a family whose thread owns P consecutive 16-byte packs: the frame of
// the four kernels of a GRID FIELD objective (grid_field_kernels.cuh), whose thread owns W nodes of D = P unknowns.
//
// It is halo_eval and halo_trial with the four places that assume one pack per thread generalised: nv = n / (W*P) counts the
// threads' units, the bounds and g0 are loaded and x and g stored as the packs vi*P + q, q < P, own(Loads, q) is pack q of the
// lane's own, and pack() fills Pack<T> (&g)[P].  Everything else -- the loops, the BOUNDED conventions, the outputs, the tile
// order, the reductions, the completion signal, the tail's order and what a family F supplies -- is halo_frame.cuh's, which
// describes it; F also has
//     static constexpr int P                               the packs a thread owns: [vi*P, vi*P + P)
// and its Pos counts in units of W coordinates per thread (the frame's flat steps are vi*W: nodes, for a grid field).
//
// Why a second frame and not a parameter of the first: with the packs-per-thread count in halo_frame.cuh and P = 1 in its five
// families the source of every existing kernel is equivalent, but not its registers.  Where the reference to the lane's own
// pack is taken relative to pack(), a loop of one trip over the packs, a lambda per pack: each moved the VGPR count of some
// existing kernel by 2 to 11 (k_volume_eval f32 216 -> 207, k_grid_b_dg_maxstep_trial f32 156 -> 152 or 158,
// k_chain_b_dg_maxstep_trial f64 146 -> 150, ...; occupancy and scratch unchanged), and a form that restored one moved another.
// The existing kernels keep their frame, text and registers (profiles/own_frame_kernel_resources.tsv).
#pragma once
#include "halo_frame.cuh"

namespace lbfgsx {

// ---------------------------------------------------------------- k_eval's and k_b_eval's counterparts
// BOUNDED false: out[0] = f(x), out[1] = g.g, out[2] = x.x;  true: out[0] = f(x), out[1] = x.x, out[2] = ||P(x-g)-x||_inf
template <class T, class F, class OBJ, bool BOUNDED>
__device__ __forceinline__ void halo_field_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb,
                                                const T* __restrict__ ub, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, P = F::P;
    constexpr int NA = BOUNDED ? 2 : 3, XX = NA - 1;  // acc[0]: f's sum, acc[XX]: x.x, acc[1] of three: g.g
    A acc[NA];
    double pgm = 0.0;
    const int64_t nv = n / (W * P);
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int lane = threadIdx.x & 63;
    auto ld = [&](int64_t i) { return x[i]; };
    const typename F::Pos step = F::pos(obj, stride * W);
    typename F::Pos pos = F::pos(obj, (int64_t(blockIdx.x) * kBlock + threadIdx.x) * W);
    for (int64_t v0 = int64_t(blockIdx.x) * kBlock + (threadIdx.x - lane); v0 < nv; v0 += stride)
    {
        const int64_t vi = v0 + lane;
        typename F::Loads xv;
        Pack<T> pl[P], pu[P];
        F::load(x, vi, nv, n, obj, xv);
        if constexpr (BOUNDED)
            if (vi < nv)
            {
#pragma unroll
                for (int q = 0; q < P; q++)
                {
                    pl[q] = ldv(lb, vi * P + q);
                    pu[q] = ldv(ub, vi * P + q);
                }
            }
        F::gather(xv, vi, nv, n, obj, ld, [&](const auto&... win) __attribute__((always_inline)) {
            if (vi >= nv)
                return;
            Pack<T> pg[P];
            F::pack(obj, vi, n, pos, pg, acc[0], win...);
#pragma unroll
            for (int q = 0; q < P; q++)
            {
                const Pack<T>& px = F::own(xv, q);
                stv(g, vi * P + q, pg[q]);
#pragma unroll
                for (int k = 0; k < W; k++)
                {
                    acc[XX].add_prod(px.e[k], px.e[k]);
                    if constexpr (BOUNDED)
                        pgm = fmax(pgm, double(projg_term(px.e[k], pg[q].e[k], pl[q].e[k], pu[q].e[k])));
                    else
                        acc[1].add_prod(pg[q].e[k], pg[q].e[k]);
                }
            }
        });
        F::advance(obj, pos, step);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * (W * P); i < n; i++)
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
__device__ __forceinline__ void halo_field_trial(const T* __restrict__ xp, const T* __restrict__ g0, const T* __restrict__ d,
                                                 const T* __restrict__ lb, const T* __restrict__ ub, T step, T* __restrict__ x,
                                                 T* __restrict__ g, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out, int rev)
{
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W, U = F::U, P = F::P;
    constexpr int NA = BOUNDED ? 3 : 2;
    A acc[NA];  // f's sum, grad(x).d, g0.d
    double smin = __longlong_as_double(0x7FF0000000000000ll);
    auto feas = [&](T xi, T di, T lo, T up) __attribute__((always_inline)) {
        if (di > T(0))
            smin = fmin(smin, double((up - xi) / di) + 0.0);
        else if (di < T(0))
            smin = fmin(smin, double((lo - xi) / di) + 0.0);
    };
    const int64_t nv = n / (W * P);
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
        Pack<T> pg0[U][P], plo[U][P], pup[U][P];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            F::load(xp, vi, nv, n, obj, lxp[u]);
            F::load(d, vi, nv, n, obj, ldd[u]);
            if constexpr (BOUNDED)
                if (vi < nv)
                {
#pragma unroll
                    for (int q = 0; q < P; q++)
                    {
                        pg0[u][q] = ldv<T>(g0, vi * P + q);
                        plo[u][q] = ldv<T>(lb, vi * P + q);
                        pup[u][q] = ldv<T>(ub, vi * P + q);
                    }
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
                Pack<T> pg[P];
                if constexpr (BOUNDED)
                {
#pragma unroll
                    for (int q = 0; q < P; q++)
                    {
                        const Pack<T>& pxp = F::own(lxp[u], q);
                        const Pack<T>& pd = F::own(ldd[u], q);
#pragma unroll
                        for (int k = 0; k < W; k++)
                        {
                            if constexpr (U == 1)
                            {
                                // the bounds by value, read first: as operands of feas the two reads are sunk into the branches on
                                // d's sign and, at this depth (k_volume_b_dg_maxstep_trial), lb's and ub's packs then live in 48
                                // bytes of scratch.  The deeper tiles keep the statements they were measured with
                                const T lo = plo[u][q].e[k], up = pup[u][q].e[k];
                                acc[NA - 1].add_prod(pg0[u][q].e[k], pd.e[k]);
                                feas(pxp.e[k], pd.e[k], lo, up);
                            }
                            else
                            {
                                acc[NA - 1].add_prod(pg0[u][q].e[k], pd.e[k]);
                                feas(pxp.e[k], pd.e[k], plo[u][q].e[k], pup[u][q].e[k]);
                            }
                        }
                    }
                }
                F::pack(obj, vi, n, pos, pg, acc[0], win...);
#pragma unroll
                for (int q = 0; q < P; q++)
                {
                    const Pack<T>& pd = F::own(ldd[u], q);
                    stv<T>(x, vi * P + q, F::own(xv, q));
                    stv<T>(g, vi * P + q, pg[q]);
#pragma unroll
                    for (int k = 0; k < W; k++)
                        acc[1].add_prod(pg[q].e[k], pd.e[k]);
                }
            });
            F::advance(obj, pos, ustep);
        }
        if (rev)
            F::retreat(obj, pos0, tstep);
        else
            F::advance(obj, pos0, tstep);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * (W * P); i < n; i++)
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
