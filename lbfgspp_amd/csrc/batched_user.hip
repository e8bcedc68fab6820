// lbfgspp_amd/csrc/batched_user.hip -- the lock-step batch around a user objective that sees the batch as ONE packed array
// (lbfgsx_lockstep_minimize_fn, include/lbfgsx_solver.h).
//
// The batch keeps its vectors point-major ([3][P][ld]) and every problem's trial in its own point slot, so the rows of the
// problems that evaluate in one lock-step turn are neither adjacent nor in one slot.  A callback that wants "row k = the k-th
// evaluating problem" gets a packed copy, made by the statements that surround the evaluation anyway:
//   kb_pack    x(x_out) = x(x_in) + step * drt   written to the point slot and to packed row col_u      (kb_point + a copy)
//   kb_unpack  packed gradient row col_u -> gradient slot of x_out, grad . drt in the same pass         (a copy + kb_gdot)
// Element-wise arithmetic and accumulators are those of kb_point / kb_gdot (batched.hip), the sums go through bat_reduce:
// a batch member's trajectory is that of POINT + caller-fills-slot + GDOT, bit for bit.  Launch and descriptor conventions
// are lbfgsx_bat_launch's: grid = (blocks per problem, problems), one lbfgsx_bat_desc per problem staged in host-mapped
// memory, results through the host-mapped table.  16-byte accesses, tiles of U x kBlock vectors as in kb_trial.
#include <algorithm>
#include <vector>

#include "batched.hpp"

namespace lbfgsx {

template <class T>
__global__ void __launch_bounds__(kBlock) kb_pack(BatBufs<T> b, const BatDesc* __restrict__ desc, T* __restrict__ UX, int64_t n)
{
    const int p = blockIdx.y;
    const BatDesc de = desc[p];
    if (!de.active)
        return;
    constexpr int W = Vec16<T>::W;
    const T* xp = b.x(de.x_in, p);
    const T* d = b.d(p);
    T* x = b.x(de.x_out, p);
    T* row = UX + int64_t(de.col_u) * b.ld;
    const T step = T(de.step);
    const int64_t nv = n / W;
    constexpr int U = 4;
    const int64_t tile = int64_t(kBlock) * U;
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = t0 + threadIdx.x;
        Pack<T> pxp[U], pd[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (base + u * kBlock < nv)
            {
                pxp[u] = ldv(xp, base + u * kBlock);
                pd[u] = ldv(d, base + u * kBlock);
            }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                Pack<T> px;
#pragma unroll
                for (int k = 0; k < W; k++)
                    px.e[k] = pxp[u].e[k] + step * pd[u].e[k];
                stv(x, vi, px);
                stv(row, vi, px);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T xi = xp[i] + step * d[i];
            x[i] = xi;
            row[i] = xi;
        }
}

// out (per problem, at sc[i_out]): g(x_out) . d, where g(x_out) is what this pass copies from packed row col_u
template <class T>
__global__ void __launch_bounds__(kBlock) kb_unpack(BatBufs<T> b, const BatDesc* __restrict__ desc, const T* __restrict__ UG,
                                                    int64_t n, BatWs ws)
{
    const int p = blockIdx.y;
    const BatDesc de = desc[p];
    if (!de.active)
        return;
    typedef typename AccOf<T>::type A;
    constexpr int W = Vec16<T>::W;
    const T* row = UG + int64_t(de.col_u) * b.ld;
    const T* d = b.d(p);
    T* g = b.g(de.x_out, p);
    A acc[1];
    const int64_t nv = n / W;
    constexpr int U = 4;
    const int64_t tile = int64_t(kBlock) * U;
    for (int64_t t0 = int64_t(blockIdx.x) * tile; t0 < nv; t0 += int64_t(gridDim.x) * tile)
    {
        const int64_t base = t0 + threadIdx.x;
        Pack<T> pg[U], pd[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (base + u * kBlock < nv)
            {
                pg[u] = ldv(row, base + u * kBlock);
                pd[u] = ldv(d, base + u * kBlock);
            }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int64_t vi = base + u * kBlock;
            if (vi < nv)
            {
                stv(g, vi, pg[u]);
#pragma unroll
                for (int k = 0; k < W; k++)
                    acc[0].add_prod(pg[u].e[k], pd[u].e[k]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * W; i < n; i++)
        {
            const T gi = row[i];
            g[i] = gi;
            acc[0].add_prod(gi, d[i]);
        }
    if (bat_reduce<1>(acc, ws) && threadIdx.x == 0)
    {
        T* o = b.scal(p) + de.i_out;
        o[0] = T(acc[0].value());
        bat_result(ws, p, 0, double(o[0]));
        bat_signal(ws);
    }
}

// The descriptors of a pack / unpack launch index device memory: check them before anything is launched.
static int user_desc_check(const lbfgsx_batch* c, const lbfgsx_bat_desc* desc, const char* who, int* nactive)
{
    std::vector<char> taken(size_t(c->P), 0);
    int na = 0;
    for (int p = 0; p < c->P; p++)
    {
        const lbfgsx_bat_desc& d = desc[p];
        if (!d.active)
            continue;
        const bool ok = d.x_in >= 0 && d.x_in <= 2 && d.x_out >= 0 && d.x_out <= 2 && d.x_in != d.x_out && d.col_u >= 0 &&
                        d.col_u < c->P && !taken[size_t(d.col_u)] && d.i_out >= 0 && d.i_out < c->scn;
        if (!ok)
        {
            set_error(std::string(who) + ": descriptor of problem " + std::to_string(p) +
                      " names a point outside 0..2, x_in == x_out, a packed row outside the batch or taken twice, or a scalar "
                      "index outside the table");
            return LBFGSX_E_INVALID;
        }
        taken[size_t(d.col_u)] = 1;
        na++;
    }
    *nactive = na;
    return LBFGSX_OK;
}

// blocks per problem of a launch that `nactive` problems take part in (the rule of lbfgsx_bat_launch)
static int user_grid_x(const lbfgsx_batch* c, int nactive)
{
    const int64_t w = (c->dtype == LBFGSX_F64) ? 2 : 4;
    const int64_t tiles = std::max<int64_t>(1, (c->n / w + 4 * kBlock - 1) / (4 * kBlock));
    return int(std::max<int64_t>(c->gx, std::min<int64_t>(std::min<int64_t>(1024 / nactive, kBatGxMax), tiles)));
}

static int user_alloc(lbfgsx_batch* c)
{
    if (c->UX && c->UG)
        return LBFGSX_OK;
    const size_t vb = size_t(c->ld) * c->esz * size_t(c->P);
    if (!c->UX)
        LBFGSX_HIP(hipMalloc(&c->UX, vb));
    if (!c->UG)
        LBFGSX_HIP(hipMalloc(&c->UG, vb));
    return LBFGSX_OK;
}

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

void* lbfgsx_bat_packed(lbfgsx_batch* c, int kind)
{
    if (!c || (kind != 0 && kind != 1))
        return nullptr;
    lbfgsx::DeviceGuard dev_guard_(c->device);
    if (user_alloc(c) != LBFGSX_OK)
        return nullptr;
    return kind == 0 ? c->UX : c->UG;
}

int lbfgsx_bat_pack(lbfgsx_batch* c, const lbfgsx_bat_desc* desc)
{
    if (!c || !desc)
    {
        set_error("lbfgsx_bat_pack: null argument");
        return LBFGSX_E_INVALID;
    }
    int nactive = 0;
    const int rc = user_desc_check(c, desc, "lbfgsx_bat_pack", &nactive);
    if (rc != LBFGSX_OK || nactive == 0)
        return rc;
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const int ra = user_alloc(c);
    if (ra != LBFGSX_OK)
        return ra;
    const void* dd = nullptr;
    LBFGSX_HIP(lbfgsx::bat_stage(c, desc, sizeof(BatDesc) * size_t(c->P), &dd));
    const dim3 grid(unsigned(user_grid_x(c, nactive)), unsigned(c->P));
    BAT_DISPATCH(c, {
        BAT_LAUNCH(c, (kb_pack<T>), grid, dim3(kBlock), 0, c->stream, bufs<T>(c), static_cast<const BatDesc*>(dd),
                   static_cast<T*>(c->UX), c->n);
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}

int lbfgsx_bat_unpack(lbfgsx_batch* c, const lbfgsx_bat_desc* desc, double* out)
{
    if (!c || !desc || !out)
    {
        set_error("lbfgsx_bat_unpack: null argument");
        return LBFGSX_E_INVALID;
    }
    int nactive = 0;
    const int rc = user_desc_check(c, desc, "lbfgsx_bat_unpack", &nactive);
    if (rc != LBFGSX_OK || nactive == 0)
        return rc;
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const int ra = user_alloc(c);
    if (ra != LBFGSX_OK)
        return ra;
    const void* dd = nullptr;
    LBFGSX_HIP(lbfgsx::bat_stage(c, desc, sizeof(BatDesc) * size_t(c->P), &dd));
    const dim3 grid(unsigned(user_grid_x(c, nactive)), unsigned(c->P));
    const BatWs ws = lbfgsx::bat_arm(c, nactive);
    BAT_DISPATCH(c, {
        BAT_LAUNCH(c, (kb_unpack<T>), grid, dim3(kBlock), 0, c->stream, bufs<T>(c), static_cast<const BatDesc*>(dd),
                   static_cast<const T*>(c->UG), c->n, ws);
    });
    LBFGSX_HIP(hipGetLastError());
    LBFGSX_HIP(lbfgsx::bat_wait(c));
    const volatile double* tab = c->res_host;
    for (int p = 0; p < c->P; p++)
        if (desc[p].active)
            out[p] = tab[size_t(p) * kBatRes];
    return LBFGSX_OK;
}

int lbfgsx_bat_set_x0(lbfgsx_batch* c, const void* src)
{
    if (!c || !src)
    {
        set_error("lbfgsx_bat_set_x0: null argument");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    lbfgsx::counters().copies.fetch_add(1, std::memory_order_relaxed);
    const size_t row = size_t(c->n) * c->esz;
    LBFGSX_HIP(hipMemcpy2DAsync(c->X, size_t(c->ld) * c->esz, src, row, row, size_t(c->P), hipMemcpyDefault, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));  // src is the caller's: it may go when this returns
    c->stage_unwaited = 0;
    return LBFGSX_OK;
}

int lbfgsx_bat_device_push(const lbfgsx_batch* c, int* prev)
{
    int cur = -1;
    if (!c || !prev)
    {
        set_error("lbfgsx_bat_device_push: null argument");
        return LBFGSX_E_INVALID;
    }
    LBFGSX_HIP(hipGetDevice(&cur));
    *prev = cur;
    if (cur != c->device)
        LBFGSX_HIP(hipSetDevice(c->device));
    return LBFGSX_OK;
}
}
