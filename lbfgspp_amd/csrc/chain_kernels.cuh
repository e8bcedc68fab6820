// lbfgspp_amd/csrc/chain_kernels.cuh -- the four evaluation kernels for a CHAIN objective
//     f(x) = sum over t = 0 .. n-K of phi(x[t], .., x[t+K-1]; t),   K = 2 or 3,
// one term starting at every coordinate, so that neighbouring terms overlap (include/lbfgsx.h, "chain objectives").
//
// k_chain_eval, k_chain_trial, k_chain_b_eval and k_chain_b_dg_maxstep_trial take the arguments of k_eval, k_trial, k_b_eval
// and k_b_dg_maxstep_trial (lbfgs_kernels.cuh, lbfgsb_kernels.cuh) and are launched with their grids: the same outputs,
// tiles, tile order, reductions and completion signal; launch_args.hpp serves both families.  They are halo_eval and
// halo_trial (halo_frame.cuh) around ChainFamily, at the end of this file: the frame holds the loops, the bounds, the sums
// and the tail's order; this file holds what a chain loads, how its window is put together and the terms of a pack.  They
// are compiled at run time only (jit_objective.hip): OBJ is the struct generated around the caller's text for one term,
//     static constexpr int K;   T term(const T (&x)[K], T (&g)[K], int64_t t) const;
//
// Ownership.  The thread that owns coordinate j writes grad[j] and adds the value of the term that STARTS at j (if one
// does: j <= n-K) to f's accumulator, once.  grad[j] is the sum of g_t[j-t] over t = max(0, j-K+1) .. min(j, n-K) in
// ascending t, started from the first contribution (no leading 0 +).  A thread owns the W coordinates of a 16-byte pack
// [b, b+W); thread 0 of block 0 also owns the coordinates past the last whole pack.  So a thread evaluates the terms that
// start at b-(K-1) .. b+W-1, clipped to [0, n-K], from a window of W + 2(K-1) values of x.
//
// The window.  In all four kernels adjacent lanes hold adjacent packs, so the K-1 values on either side come from the
// neighbouring lanes by cross-lane moves, which run with all 64 lanes of the wave in the loop (the frame's loops run on the
// wave's first pack, not the lane's).  Only a lane without a neighbour reads memory: lane 0 of a wave to its left, lane 63
// and the lane that holds the last whole pack to their right (there the halo may be tail coordinates).  Those reads are
// issued with the pack's own loads.  In the trial kernels a halo value is the neighbour's computed xp + step*d or the same
// statement on halo loads of xp and d -- never a read of the x this launch writes.
// No index below 0 or at or above n is loaded, and a term that does not lie inside [0, n) is not evaluated, so the text of a
// term may read p0[i] .. p0[i+K-1].
#pragma once
#include "halo_frame.cuh"

namespace lbfgsx {

// The coordinate whose value slot j of a lane's spare halo registers holds, or -1: lane 0 fetches x[b-H+j], another lane
// without a right neighbour x[b+W+j]; lane 0 without a right neighbour fetches that side when the window is put together
// (chain_window's `late`)
template <class T, int K>
__device__ __forceinline__ int64_t chain_edge_index(int64_t vi, int64_t nv, int64_t n, int j)
{
    constexpr int W = Vec16<T>::W, H = K - 1;
    const int lane = threadIdx.x & 63;
    if (vi >= nv)
        return -1;
    int64_t idx = -1;
    if (lane == 0)
        idx = vi * W - H + j;
    else if (lane == 63 || vi + 1 >= nv)
        idx = vi * W + W + j;
    return (idx >= 0 && idx < n) ? idx : -1;
}

// xw[0 .. W+2H) = x[b-H .. b+W+H) around the pack px at vi.  Called by all 64 lanes of the wave, whether they hold a pack
// or not (a lane past the end hands its neighbour values nobody uses).  edge: the values at chain_edge_index's coordinates
// (anything where it said -1: the terms that would read them are not evaluated); late(j): x[b+W+j] from memory, or anything
// when that coordinate is not below n.
template <class T, int K, class LATE>
__device__ __forceinline__ void chain_window(const Pack<T>& px, const T (&edge)[K - 1], int64_t vi, int64_t nv, LATE late,
                                             T (&xw)[Vec16<T>::W + 2 * (K - 1)])
{
    constexpr int W = Vec16<T>::W, H = K - 1;
    static_assert(H >= 1 && H <= W, "the halo of a pack lies inside the neighbouring pack");
    const int lane = threadIdx.x & 63;
    const bool mem_r = lane == 63 || vi + 1 >= nv;
#pragma unroll
    for (int j = 0; j < H; j++)
    {
        const T up = __shfl_up(px.e[W - H + j], 1, 64);
        const T dn = __shfl_down(px.e[j], 1, 64);
        xw[j] = (lane == 0) ? edge[j] : up;
        xw[H + W + j] = mem_r ? edge[j] : dn;
    }
    if (lane == 0 && mem_r && vi < nv)
    {
#pragma unroll
        for (int j = 0; j < H; j++)
            xw[H + W + j] = late(j);
    }
#pragma unroll
    for (int k = 0; k < W; k++)
        xw[H + k] = px.e[k];
}

// the terms of one pack from its window: gradient of the pack's W coordinates, values of the terms that start inside it.
// ALL: every term b-H .. b+W-1 exists (a pack away from both ends of x)
template <bool ALL, class T, class OBJ, class A>
__device__ __forceinline__ void chain_terms(const OBJ& obj, int64_t b, int64_t n, const T (&xw)[Vec16<T>::W + 2 * (OBJ::K - 1)],
                                            Pack<T>& g, A& fx)
{
    constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    bool has[W];
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        has[k] = false;
        g.e[k] = T(0);
    }
#pragma unroll
    for (int s = 0; s < W + H; s++)
    {
        const int64_t t = b - H + s;
        if (ALL || (t >= 0 && t + K <= n))
        {
            T tx[K], tg[K];
#pragma unroll
            for (int j = 0; j < K; j++)
                tx[j] = xw[s + j];
            const T v = obj.term(tx, tg, t);
#pragma unroll
            for (int j = K - 1; j >= 0; j--)
            {
                const int k = s + j - H;  // the pack's coordinate that tg[j] belongs to
                if (k >= 0 && k < W)
                {
                    g.e[k] = has[k] ? g.e[k] + tg[j] : tg[j];
                    has[k] = true;
                }
            }
            if (s >= H)
                fx.add(v);
        }
    }
}

template <class T, class OBJ, class A>
__device__ __forceinline__ void chain_pack(const OBJ& obj, int64_t vi, int64_t n, const T (&xw)[Vec16<T>::W + 2 * (OBJ::K - 1)],
                                           Pack<T>& g, A& fx)
{
    constexpr int W = Vec16<T>::W, H = OBJ::K - 1;
    const int64_t b = vi * W;
    if (b >= H && b + W + H <= n)
        chain_terms<true>(obj, b, n, xw, g, fx);
    else
        chain_terms<false>(obj, b, n, xw, g, fx);
}

// a coordinate past the last whole pack (thread 0 of block 0): its gradient, returned, and the value of the term that starts
// there.  ld(k) = x[k] for k in [0, n) -- from memory in the evaluation kernels, recomputed from xp and d in the trial kernels
template <class T, class OBJ, class LD, class A>
__device__ __forceinline__ T chain_tail(const OBJ& obj, int64_t i, int64_t n, LD ld, A& fx)
{
    constexpr int K = OBJ::K;
    T gi = T(0);
    bool has = false;
#pragma unroll
    for (int o = K - 1; o >= 0; o--)  // the term that starts o coordinates before i: ascending t
    {
        const int64_t t = i - o;
        if (t >= 0 && t + K <= n)
        {
            T tx[K], tg[K];
#pragma unroll
            for (int j = 0; j < K; j++)
                tx[j] = ld(t + j);
            const T v = obj.term(tx, tg, t);
            gi = has ? gi + tg[o] : tg[o];
            has = true;
            if (o == 0)
                fx.add(v);
        }
    }
    return gi;
}

// the frame's family (halo_frame.cuh): one row of halo K - 1, no position to carry
template <class T, class OBJ>
struct ChainFamily
{
    static constexpr int K = OBJ::K, W = Vec16<T>::W, H = K - 1;
    static constexpr int U = 4;
    // a lane's pack and the values at chain_edge_index's coordinates.  edge stands first: with the pack first k_chain_trial
    // at K = 3 in f32 compiles to 3 waves per SIMD instead of the 4 it had (profiles/own_frame_kernel_resources.tsv)
    struct Loads
    {
        T edge[H];
        Pack<T> p;
    };
    struct Pos
    {
    };
    __device__ __forceinline__ static Pos pos(const OBJ&, int64_t) { return {}; }
    __device__ __forceinline__ static void advance(const OBJ&, Pos&, const Pos&) {}
    __device__ __forceinline__ static void retreat(const OBJ&, Pos&, const Pos&) {}

    __device__ __forceinline__ static void load(const T* __restrict__ v, int64_t vi, int64_t nv, int64_t n, const OBJ&,
                                                Loads& o)
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            o.p.e[k] = T(0);
        if (vi < nv)
            o.p = ldv(v, vi);
#pragma unroll
        for (int j = 0; j < H; j++)
        {
            const int64_t e = chain_edge_index<T, K>(vi, nv, n, j);
            o.edge[j] = T(0);
            if (e >= 0)
                o.edge[j] = v[e];
        }
    }
    __device__ __forceinline__ static void axpy(const Loads& xp, const Loads& d, T step, Loads& x)
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            x.p.e[k] = xp.p.e[k] + step * d.p.e[k];
#pragma unroll
        for (int j = 0; j < H; j++)
            x.edge[j] = xp.edge[j] + step * d.edge[j];
    }
    __device__ __forceinline__ static const Pack<T>& own(const Loads& l) { return l.p; }
    template <class LD, class BODY>
    __device__ __forceinline__ static void gather(const Loads& xv, int64_t vi, int64_t nv, int64_t n, const OBJ&, LD ld,
                                                  BODY body)
    {
        T xw[W + 2 * H];
        chain_window<T, K>(xv.p, xv.edge, vi, nv,
                           [&](int j) {
                               const int64_t e = vi * W + W + j;
                               return (e < n) ? ld(e) : T(0);
                           },
                           xw);
        body(xw);
    }
    template <class A>
    __device__ __forceinline__ static void pack(const OBJ& obj, int64_t vi, int64_t n, const Pos&, Pack<T>& g, A& fx,
                                                const T (&xw)[W + 2 * H])
    {
        chain_pack(obj, vi, n, xw, g, fx);
    }
    template <class LD, class A>
    __device__ __forceinline__ static T tail(const OBJ& obj, int64_t i, int64_t n, LD ld, A& fx)
    {
        return chain_tail<T>(obj, i, n, ld, fx);
    }
};

LBFGSX_FRAME_KERNELS(k_chain, halo_eval, halo_trial, ChainFamily<T, OBJ>)

}  // namespace lbfgsx
