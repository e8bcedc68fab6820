// lbfgspp_amd/csrc/frame_kernels.cuh -- the four __global__ kernels of a family on a kernel frame (own_frame.cuh,
// halo_frame.cuh), defined once.
//
// LBFGSX_FRAME_KERNELS(PREFIX, EVAL, TRIAL, family) defines PREFIX_eval, PREFIX_trial, PREFIX_b_eval and
// PREFIX_b_dg_maxstep_trial with the parameter lists of k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial (OBJ after n):
// launch_args.hpp serves all the families.  EVAL and TRIAL are the frame's two functions, <T, family, OBJ, BOUNDED>; the
// family goes last because it may hold a comma (ChainFamily<T, OBJ>).
#pragma once

#define LBFGSX_FRAME_KERNELS(PREFIX, EVAL, TRIAL, ...)                                                                         \
    template <class T, class OBJ>                                                                                              \
    __global__ void __launch_bounds__(kBlock)                                                                                  \
        PREFIX##_eval(const T* __restrict__ x, T* __restrict__ g, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out)           \
    {                                                                                                                          \
        EVAL<T, __VA_ARGS__, OBJ, false>(x, g, nullptr, nullptr, n, obj, ws, out);                                             \
    }                                                                                                                          \
    template <class T, class OBJ>                                                                                              \
    __global__ void __launch_bounds__(kBlock)                                                                                  \
        PREFIX##_b_eval(const T* __restrict__ x, T* __restrict__ g, const T* __restrict__ lb, const T* __restrict__ ub,        \
                        int64_t n, OBJ obj, RedWs ws, T* __restrict__ out)                                                     \
    {                                                                                                                          \
        EVAL<T, __VA_ARGS__, OBJ, true>(x, g, lb, ub, n, obj, ws, out);                                                        \
    }                                                                                                                          \
    template <class T, class OBJ>                                                                                              \
    __global__ void __launch_bounds__(kBlock)                                                                                  \
        PREFIX##_trial(const T* __restrict__ xp, const T* __restrict__ d, T step, T* __restrict__ x, T* __restrict__ g,        \
                       int64_t n, OBJ obj, RedWs ws, T* __restrict__ out, int rev)                                             \
    {                                                                                                                          \
        TRIAL<T, __VA_ARGS__, OBJ, false>(xp, nullptr, d, nullptr, nullptr, step, x, g, n, obj, ws, out, rev);                 \
    }                                                                                                                          \
    template <class T, class OBJ>                                                                                              \
    __global__ void __launch_bounds__(kBlock)                                                                                  \
        PREFIX##_b_dg_maxstep_trial(const T* __restrict__ xp, const T* __restrict__ g0, const T* __restrict__ d,               \
                                    const T* __restrict__ lb, const T* __restrict__ ub, T step, T* __restrict__ x,             \
                                    T* __restrict__ g, int64_t n, OBJ obj, RedWs ws, T* __restrict__ out, int rev)             \
    {                                                                                                                          \
        TRIAL<T, __VA_ARGS__, OBJ, true>(xp, g0, d, lb, ub, step, x, g, n, obj, ws, out, rev);                                 \
    }
