// lbfgspp_amd/csrc/lbfgsb_subspace.hip -- L-BFGS-B device operators of the subspace minimisation (BOXCQP): the solve's dots, the partitions and
// checks, the fused solve + sweep passes over the free rows and over the index list of L u U, the vector statements.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#define LBFGSB_TU "lbfgsb_subspace"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

template <class T, int NC>
static int solve_dots_t(lbfgsx_ctx* c, int pmask, int vsel_id, const double* coef, double theta, int fmask, double* wty)
{
    const int total = 2 * c->ncorr;
    int which[32];
    for (int k = 0; k < total; k++)
        which[k] = k;
    const bool compact = wf_serves(c, fmask) && wf_serves(c, pmask);
    const int64_t nrows = compact ? c->bstate->wf_n : c->n;
    Cols<T, 32> cl = compact ? wf_cols<T>(c, total) : col_list<T, 32>(c, which, total);
    CoefArg<T> cf;
    for (int k = 0; k < 80; k++)
        cf.c[k] = (coef && k < total) ? T(coef[k]) : T(0);
    const int grid = std::min(c->grid_for(nrows), lbfgsb_state::kDotsGrid);
    LBFGSX_LAUNCH((k_solve_dots<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, cl, total, bvecs<T>(c), vsel_id, cf,
                       coef ? 1 : 0, pmask, fmask, T(theta), nrows, c->ws, c->bstate->dout,
                       compact ? c->bstate->wf_idx : static_cast<const int*>(nullptr));
    LBFGSX_HIP(hipGetLastError());
    double r[NC];
    int rc = fetch_doubles(c, NC, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
        wty[k] = r[k];
    return LBFGSX_OK;
}
template <class T, int NC>
static int solve_sweep_t(lbfgsx_ctx* c, int first, int vsel_id, const double* coef, double theta, double* wty, double* sums,
                         unsigned lu_cap_now, int* lu_dst)
{
    const int total = 2 * c->ncorr;
    int which[32];
    for (int k = 0; k < total; k++)
        which[k] = k;
    // the rows this pass acts on are the free rows: from their compact copy when the Gram pass before it left one
    lbfgsb_state* b = c->bstate;
    const bool compact = wf_serves(c, ST_FREE);
    const int64_t nrows = compact ? b->wf_n : c->n;
    const int* ridx = compact ? b->wf_idx : nullptr;
    Cols<T, 32> cl = compact ? wf_cols<T>(c, total) : col_list<T, 32>(c, which, total);
    CoefArg<T> cf;
    for (int k = 0; k < 80; k++)
        cf.c[k] = (coef && k < total) ? T(coef[k]) : T(0);
    const int grid = std::min(c->grid_for(nrows), lbfgsb_state::kDotsGrid);
    // compact vectors: the first solve over the compact copy starts them (when an index list of L u U will let the sweeps
    // that follow stay on the fused path), the later solves use them
    int cv = 0;
    if (first)
    {
        b->cv_live = false;
        if (compact && b->cv_use && lu_cap_now > 0 && (vsel_id == VS_NEG_CF || vsel_id == VS_NEG_RHS || vsel_id == VS_Y) &&
            cv_alloc(c) == LBFGSX_OK)
            cv = 1;
    }
    else if (b->cv_live)
    {
        if (compact && (vsel_id == VS_NEG_CF || vsel_id == VS_NEG_RHS || vsel_id == VS_Y))
            cv = 2;
        else
        {
            const int rcb = cv_back(c, false);
            if (rcb)
                return rcb;
        }
    }
    T* cli = nullptr;
    T* cui = nullptr;
    const BVecs<T> full = bvecs<T>(c);
    const BVecs<T> cvb = cv ? bvecs_cv<T>(c, &cli, &cui) : full;
    lbfgsx::poll_arm(c);
    if (first)
        LBFGSX_LAUNCH((k_solve_sweep<T, NC, 1>), dim3(grid), dim3(kBlock), 0, c->stream, cl, total, full, cvb, vsel_id, cf,
                      coef ? 1 : 0, T(theta), nrows, c->ws, b->dout, lu_dst, b->lu_cnt, lu_cap_now, ridx, cli, cui, cv);
    else
        LBFGSX_LAUNCH((k_solve_sweep<T, NC, 0>), dim3(grid), dim3(kBlock), 0, c->stream, cl, total, cv ? cvb : full, cvb, vsel_id, cf,
                      coef ? 1 : 0, T(theta), nrows, c->ws, b->dout, lu_dst, b->lu_cnt, lu_cap_now, ridx, cli, cui, cv);
    if (cv == 1)
    {
        b->cv_live = true;
        b->cv_starts++;
        count_cv_start();
    }
    LBFGSX_HIP(hipGetLastError());
    const int nd = first ? 0 : NC;
    double r[NC + 7];
    int rc = fetch_doubles(c, nd + 7, r);
    if (rc)
        return rc;
    if (!first)
        for (int k = 0; k < total; k++)
            wty[k] = r[k];
    for (int k = 0; k < 7; k++)
        sums[k] = r[nd + k];
    return LBFGSX_OK;
}
// the same through kx_solve_sweep (any 2c <= 80)
template <class T>
static int solve_sweep_x(lbfgsx_ctx* c, int first, int vsel_id, const double* coef, double theta, double* wty, double* sums,
                         unsigned lu_cap_now, int* lu_dst, const double* rc1 = nullptr, const double* rc2 = nullptr)
{
    const int total = 2 * c->ncorr;
    lbfgsb_state* b = c->bstate;
    const bool compact = wf_serves(c, ST_FREE);
    const int64_t nrows = compact ? b->wf_n : c->n;
    const int* ridx = compact ? b->wf_idx : nullptr;
    const ColsX<T> cl = compact ? colsx_wf<T>(c, total) : colsx_full<T>(c, total);
    CoefX<T> cf;
    for (int k = 0; k < kColsX; k++)
        cf.c[k] = (coef && k < total) ? T(coef[k]) : T(0);
    int cv = 0;
    if (first)
    {
        b->cv_live = false;
        if (compact && b->cv_use && lu_cap_now > 0 && (vsel_id == VS_NEG_CF || vsel_id == VS_NEG_RHS || vsel_id == VS_Y) &&
            cv_alloc(c) == LBFGSX_OK)
            cv = 1;
    }
    else if (b->cv_live)
    {
        if (compact && (vsel_id == VS_NEG_CF || vsel_id == VS_NEG_RHS || vsel_id == VS_Y))
            cv = 2;
        else
        {
            const int rcb = cv_back(c, false);
            if (rcb)
                return rcb;
        }
    }
    T* cli = nullptr;
    T* cui = nullptr;
    const BVecs<T> full = bvecs<T>(c);
    const BVecs<T> cvb = cv ? bvecs_cv<T>(c, &cli, &cui) : full;
    ProX<T> pro;
    pro.mode = (rc1 || rc2) ? LBFGSX_GP_RHS : LBFGSX_GP_NONE;
    pro.use1 = rc1 ? 1 : 0;
    pro.use2 = rc2 ? 1 : 0;
    if (rc1 || rc2)
        for (int k = 0; k < kColsX; k++)
        {
            pro.c1[k] = (rc1 && k < total) ? T(rc1[k]) : T(0);
            pro.c2[k] = (rc2 && k < total) ? T(rc2[k]) : T(0);
        }
    lbfgsx::poll_arm(c);
    int rc = xl::solve_sweep<T>(c->stream, b->num_cus, first, cl, total, (first || !cv) ? full : cvb, cvb, vsel_id, cf, coef ? 1 : 0,
                                T(theta), nrows, wsx(c), b->dout, lu_dst, b->lu_cnt, lu_cap_now, ridx, cli, cui, cv,
                                (rc1 || rc2) ? &pro : static_cast<const ProX<T>*>(nullptr));
    if (rc)
        return rc;
    if (cv == 1)
    {
        b->cv_live = true;
        b->cv_starts++;
        count_cv_start();
    }
    const int nd = first ? 0 : total;
    double r[kColsX + 7];
    rc = fetch_doubles(c, nd + 7, r);
    if (rc)
        return rc;
    if (!first)
        for (int k = 0; k < total; k++)
            wty[k] = r[k];
    for (int k = 0; k < 7; k++)
        sums[k] = r[nd + k];
    return LBFGSX_OK;
}

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_solve_wty(lbfgsx_ctx* c, int pmask, int vsel_id, const double* coef, double theta, int fmask, double* wty)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int total = 2 * c->ncorr;
    if (total < 1 || total > 32 || c->bstate->multidot_chunked)
    {
        set_error("lbfgsx_b_solve_wty: needs 1 <= 2*ncorr <= 32");
        return LBFGSX_E_INVALID;
    }
    DISPATCH_T(c, {
        if (total <= 8) rc = solve_dots_t<T, 8>(c, pmask, vsel_id, coef, theta, fmask, wty);
        else if (total <= 16) rc = solve_dots_t<T, 16>(c, pmask, vsel_id, coef, theta, fmask, wty);
        else if (total <= 24) rc = solve_dots_t<T, 24>(c, pmask, vsel_id, coef, theta, fmask, wty);
        else rc = solve_dots_t<T, 32>(c, pmask, vsel_id, coef, theta, fmask, wty);
    });
    return rc;
}

int lbfgsx_b_sub_partition(lbfgsx_ctx* c, int64_t* nL, int64_t* nU, int64_t* nP)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[3];
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        c->bstate->lu_valid = false;  // this partition keeps no index list
        LBFGSX_LAUNCH((k_sub_partition<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, c->n, c->ws, c->bstate->dout);
    });
    LBFGSX_HIP(hipGetLastError());
    rc = fetch_doubles(c, 3, r);
    if (rc)
        return rc;
    *nL = int64_t(r[0]);
    *nU = int64_t(r[1]);
    *nP = int64_t(r[2]);
    return LBFGSX_OK;
}

int lbfgsx_b_sub_check(lbfgsx_ctx* c, int64_t counts[4])
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[4];
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        LBFGSX_LAUNCH((k_sub_check<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, c->n, c->ws, c->bstate->dout);
    });
    LBFGSX_HIP(hipGetLastError());
    rc = fetch_doubles(c, 4, r);
    if (rc)
        return rc;
    for (int k = 0; k < 4; k++)
        counts[k] = int64_t(r[k]);
    return LBFGSX_OK;
}

int lbfgsx_b_sub_sweep_begin(lbfgsx_ctx* c, int first, int64_t* nL, int64_t* nU, int64_t* nP, int64_t counts[4])
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[7];
    // the list pays while L u U is a few thousand rows (steady state: 10^1..10^3); in the early iterations the sets hold
    // 10^5..10^6 rows and the dense scans are the better form -- decided from the size the previous partition found
    const unsigned lu_cap_now = c->bstate->lu_pred <= lbfgsb_state::kLuMax ? c->bstate->lu_cap : 0u;
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        lbfgsx::model_add(double(c->n) * (7 * sizeof(T) + 2));  // byte model: y, lam, mu, lb, ub, x0, cF and the state byte; state and rhs written
        LBFGSX_LAUNCH((k_sub_sweep_begin<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, first ? 1 : 0, c->n, c->ws,
                           c->bstate->dout, c->bstate->lu_ptr(), c->bstate->lu_cnt, lu_cap_now);
    });
    LBFGSX_HIP(hipGetLastError());
    c->bstate->lu_valid = false;
    rc = fetch_doubles(c, 7, r);
    if (rc)
        return rc;
    *nL = int64_t(r[0]);
    *nU = int64_t(r[1]);
    *nP = int64_t(r[2]);
    c->bstate->lu_pred = *nL + *nU;
    if (lu_cap_now && *nL + *nU <= int64_t(lu_cap_now))
    {
        c->bstate->lu_n = int(*nL + *nU);
        c->bstate->lu_valid = true;
    }
    for (int k = 0; k < 4; k++)
        counts[k] = int64_t(r[3 + k]);
    return LBFGSX_OK;
}

int lbfgsx_b_solve_sweep(lbfgsx_ctx* c, int first, int vsel_id, const double* coef, double theta, double* wty, int64_t sums[7])
{
    return lbfgsx_b_solve_sweep_rhs(c, first, vsel_id, coef, theta, nullptr, nullptr, wty, sums);
}

int lbfgsx_b_solve_sweep_rhs_ready(lbfgsx_ctx* c)
{
    if (!c || !c->bstate)
        return 0;
    const lbfgsb_state* b = c->bstate;
    const int total = 2 * c->ncorr;
    return (b->rhs_identity && b->split && total >= 1 && total <= kColsX && !b->multidot_chunked && b->sweep_fuse && b->lu_valid &&
            b->lu_n >= 1) ? 1 : 0;
}

int lbfgsx_b_solve_sweep_rhs(lbfgsx_ctx* c, int first, int vsel_id, const double* coef, double theta, const double* rhs_c1,
                             const double* rhs_c2, double* wty, int64_t sums[7])
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, /*keep_cv=*/first == 0);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int total = 2 * c->ncorr;
    if ((rhs_c1 || rhs_c2) && (first || vsel_id != VS_NEG_RHS || !b->split))
    {
        set_error("lbfgsx_b_solve_sweep_rhs: the rhs updates ride on a sweep's solve of -rhs (split-row kernels) only");
        return LBFGSX_E_INVALID;
    }
    if (total < 1 || total > (b->split ? kColsX : 32) || b->multidot_chunked || !b->sweep_fuse)
    {
        set_error("lbfgsx_b_solve_sweep: not available here (needs 1 <= 2*ncorr <= 80); run the separate passes");
        return LBFGSX_E_INVALID;
    }
    // selectors, before anything changes state (the compact vectors, the armed completion word): v of a fused solve is ONE
    // vector -- the bound selectors of lbfgsx_b_wtv_lu are not solved for (include/lbfgsx.h)
    if (b->split && (vsel_id == VS_LBOUND || vsel_id == VS_UBOUND))
    {
        set_error("lbfgsx_b_solve_sweep: LBFGSX_VS_LBOUND / LBFGSX_VS_UBOUND are not right-hand sides of a fused solve");
        return LBFGSX_E_INVALID;
    }
    unsigned cap;
    int* dst;
    if (first)
    {
        cap = b->lu_pred <= lbfgsb_state::kLuMax ? b->lu_cap : 0u;
        dst = b->lu_ptr();
    }
    else
    {
        // the rows of the old L and U are reached through the list of the partition that made them
        if (!b->lu_valid || b->lu_n < 1)
        {
            set_error("lbfgsx_b_solve_sweep: no index list of L u U; run the separate passes");
            return LBFGSX_E_INVALID;
        }
        cap = b->lu_cap;
        dst = b->lu_other();
    }
    double r[7];
    DISPATCH_T(c, {
        if (b->split) rc = solve_sweep_x<T>(c, first, vsel_id, coef, theta, wty, r, cap, dst, rhs_c1, rhs_c2);
        else if (total <= 8) rc = solve_sweep_t<T, 8>(c, first, vsel_id, coef, theta, wty, r, cap, dst);
        else if (total <= 16) rc = solve_sweep_t<T, 16>(c, first, vsel_id, coef, theta, wty, r, cap, dst);
        else if (total <= 20) rc = solve_sweep_t<T, 20>(c, first, vsel_id, coef, theta, wty, r, cap, dst);  // m = 10: no idle registers
        else if (total <= 24) rc = solve_sweep_t<T, 24>(c, first, vsel_id, coef, theta, wty, r, cap, dst);
        else rc = solve_sweep_t<T, 32>(c, first, vsel_id, coef, theta, wty, r, cap, dst);
    });
    if (rc)
    {
        b->lu_valid = false;
        return rc;
    }
    for (int k = 0; k < 7; k++)
        sums[k] = int64_t(r[k]);
    if (first)
    {
        b->lu_valid = false;
        b->lu_pred = sums[0] + sums[1];
        if (cap && sums[0] + sums[1] <= int64_t(cap))
        {
            b->lu_n = int(sums[0] + sums[1]);
            b->lu_valid = true;
        }
    }
    else
    {
        b->lu_pending = true;
        b->lu_pending_n = sums[0] + sums[1];
    }
    return LBFGSX_OK;
}

int lbfgsx_b_lu_sweep(lbfgsx_ctx* c, const double* coef, double theta, int64_t sums[7])
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, /*keep_cv=*/true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    if (!b->lu_pending || !b->lu_valid)
    {
        set_error("lbfgsx_b_lu_sweep: completes lbfgsx_b_solve_sweep(first = 0)");
        return LBFGSX_E_INVALID;
    }
    b->lu_pending = false;
    rc = upload_phys(c);
    if (rc)
        return rc;
    const int nl = b->lu_n;
    const int grid = std::max(1, std::min(64, (nl + kBlock - 1) / kBlock));
    const int has_w = (coef != nullptr && c->ncorr > 0) ? 1 : 0;
    double r[7];
    DISPATCH_T(c, {
        CoefArg<T> cf;
        for (int k = 0; k < 80; k++)
            cf.c[k] = (has_w && k < 2 * c->ncorr) ? T(coef[k]) : T(0);
        T* cli = nullptr;
        T* cui = nullptr;
        const BVecs<T> bv = b->cv_live ? bvecs_cv<T>(c, &cli, &cui) : bvecs<T>(c);
        lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(nl) * 64.0 * (2 * c->ncorr + 8));  // byte model: a sector per column and vector at every listed row
        LBFGSX_LAUNCH((k_lu_sweep<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, P<T>(c->S), P<T>(c->Y), c->ld,
                           b->phys_dev, c->ncorr, cf, has_w, T(theta), b->lu_ptr(), nl, c->ws, b->dout, b->lu_other(), b->lu_cnt,
                           b->lu_cap, b->cv_live ? b->wf_pos : static_cast<const int*>(nullptr), cli, cui);
    });
    LBFGSX_HIP(hipGetLastError());
    b->lu_valid = false;
    rc = fetch_doubles(c, 7, r);
    if (rc)
        return rc;
    for (int k = 0; k < 7; k++)
        sums[k] = int64_t(r[k]);
    const int64_t total = b->lu_pending_n + sums[0] + sums[1];
    b->lu_pred = total;
    b->lu_cur = 1 - b->lu_cur;
    if (total <= int64_t(b->lu_cap))
    {
        b->lu_n = int(total);
        b->lu_valid = true;
    }
    return LBFGSX_OK;
}

int lbfgsx_b_sub_op(lbfgsx_ctx* c, int op)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, /*keep_cv=*/op == SO_ASSIGN_Y);
    if (rc)
        return rc;
    if (c->bstate->cv_live)  // op == SO_ASSIGN_Y: drt = vecy on the free rows, straight from the compact y
        return cv_back(c, true);
    const int grid = c->grid_for(c->n);
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        LBFGSX_LAUNCH((k_sub_op<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, op, c->n);
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}

}  // extern "C"
