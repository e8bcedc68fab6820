// lbfgspp_amd/csrc/lbfgsb_dots.hip -- L-BFGS-B device operators, the multi-dot family: W'v under a mask or over an index list, W'd of the
// Cauchy search (with the deferred dots of the new pair), W_L'l and W_U'u, and the combinations W coef + ...
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#define LBFGSB_TU "lbfgsb_dots"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

// raw masked W'v for all 2*ncorr columns: out[0..c) = Y_j . v, out[c..2c) = S_j . v ; nnz of v inside the mask
template <class T, int NC>
static int wtv_all(lbfgsx_ctx* c, int total, int vsel_id, const T* vcol, int mask, double* out, int64_t* nnz)
{
    int which[32];
    for (int k = 0; k < total; k++)
        which[k] = k;
    Cols<T, 32> cl = col_list<T, 32>(c, which, total);
    // 2c + 1 grid reductions per launch: fewer, fatter blocks keep the reduction tail short (each thread already has
    // 2c 16-byte loads in flight)
    const int grid = std::min(c->grid_for(c->n), lbfgsb_state::kDotsGrid);
    LBFGSX_LAUNCH((k_multidot_all<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, cl, total, bvecs<T>(c), vsel_id, vcol,
                       mask, c->n, c->ws, c->bstate->dout);
    LBFGSX_HIP(hipGetLastError());
    double r[NC + 1];
    int rc = fetch_doubles(c, NC + 1, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
        out[k] = r[k];
    if (nnz)
        *nnz = int64_t(r[NC]);
    return LBFGSX_OK;
}

template <class T>
static int wtv_t(lbfgsx_ctx* c, int vsel_id, const T* vcol, int mask, double* out, int64_t* nnz)
{
    constexpr int NC = 8;
    const int total = 2 * c->ncorr;
    const int grid = c->grid_for(c->n);
    BVecs<T> b = bvecs<T>(c);
    if (c->bstate->split && total >= 1 && total <= kColsX && !c->bstate->multidot_chunked &&
        !(!vcol && c->bstate->lu_valid && mask != 0 && (mask & ~(ST_L | ST_U)) == 0 && total <= 32))
    {
        // every column in one launch, whatever 2c is (kx_multidot_mask); sets inside L u U keep the index-list kernel below
        lbfgsb_state* bs = c->bstate;
        int rc = xl::multidot_mask<T>(c->stream, bs->num_cus, colsx_full<T>(c, total), total, b, vsel_id, vcol, mask, c->n, wsx(c),
                                      bs->dout);
        if (rc)
            return rc;
        double r[kColsX + 1];
        rc = fetch_doubles(c, total + 1, r);
        if (rc)
            return rc;
        for (int k = 0; k < total; k++)
            out[k] = r[k];
        if (nnz)
            *nnz = int64_t(r[total]);
        return LBFGSX_OK;
    }
    if (!vcol && c->bstate->lu_valid && mask != 0 && (mask & ~(ST_L | ST_U)) == 0 && total <= 32)
    {
        // rows inside L u U: the index list of the last partition (k_sub_sweep_begin)
        const int nl = c->bstate->lu_n;
        const int lgrid = std::max(1, std::min(32, (nl + kBlock - 1) / kBlock));
        int which[32];
        for (int k = 0; k < total; k++)
            which[k] = k;
        Cols<T, 32> cl = col_list<T, 32>(c, which, total);
        double r[33];
        int nc_used;
#define ML_LAUNCH(N)                                                                                                        \
    do                                                                                                                      \
    {                                                                                                                       \
        LBFGSX_LAUNCH((k_multidot_list<T, N>), dim3(lgrid), dim3(kBlock), 0, c->stream, cl, total, b, vsel_id, mask,   \
                           c->bstate->lu_ptr(), nl, c->ws, c->bstate->dout);                                                \
        nc_used = N;                                                                                                        \
    } while (0)
        if (total <= 8) ML_LAUNCH(8);
        else if (total <= 16) ML_LAUNCH(16);
        else if (total <= 24) ML_LAUNCH(24);
        else ML_LAUNCH(32);
#undef ML_LAUNCH
        LBFGSX_HIP(hipGetLastError());
        int rc = fetch_doubles(c, nc_used + 1, r);
        if (rc)
            return rc;
        for (int k = 0; k < total; k++)
            out[k] = r[k];
        if (nnz)
            *nnz = int64_t(r[nc_used]);
        return LBFGSX_OK;
    }
    if (total > 8 && total <= 32 && !c->bstate->multidot_chunked)
    {
        // one launch for every column (all history columns are 16-byte aligned: ld is a multiple of 64 elements)
        if (total <= 16) return wtv_all<T, 16>(c, total, vsel_id, vcol, mask, out, nnz);
        if (total <= 24) return wtv_all<T, 24>(c, total, vsel_id, vcol, mask, out, nnz);
        return wtv_all<T, 32>(c, total, vsel_id, vcol, mask, out, nnz);
    }
    if (total == 0 && nnz)
    {
        // still count the non-zeros
        int dummy = 0;
        Cols<T, NC> cl = col_list<T, NC>(c, &dummy, 0);
        LBFGSX_LAUNCH((k_multidot<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, cl, 0, b, vsel_id, vcol, mask, c->n,
                           c->ws, c->bstate->dout);
        double r[NC + 1];
        int rc = fetch_doubles(c, NC + 1, r);
        if (rc)
            return rc;
        *nnz = int64_t(r[NC]);
        return LBFGSX_OK;
    }
    for (int first = 0; first < total; first += NC)
    {
        const int cnt = std::min(NC, total - first);
        int which[NC];
        for (int k = 0; k < cnt; k++)
            which[k] = first + k;
        Cols<T, NC> cl = col_list<T, NC>(c, which, cnt);
        LBFGSX_LAUNCH((k_multidot<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, cl, cnt, b, vsel_id, vcol, mask, c->n,
                           c->ws, c->bstate->dout);
        LBFGSX_HIP(hipGetLastError());
        double r[NC + 1];
        int rc = fetch_doubles(c, NC + 1, r);
        if (rc)
            return rc;
        for (int k = 0; k < cnt; k++)
            out[first + k] = r[k];
        if (nnz)
            *nnz = int64_t(r[NC]);
    }
    return LBFGSX_OK;
}

// p = W'd of the Cauchy search; when the dots of the last commit were deferred (lbfgsx_b_correction_dots_defer) and
// 4c reductions fit one launch, the same pass also delivers them (k_multidot2_all)
template <class T, int NC>
static int wtd2_all(lbfgsx_ctx* c, int total, const T* snew, const T* dvec, double* wtd)
{
    int which[32];
    for (int k = 0; k < total; k++)
        which[k] = k;
    Cols<T, 32> cl = col_list<T, 32>(c, which, total);
    const int grid = std::min(c->grid_for(c->n), lbfgsb_state::kDotsGrid);
    LBFGSX_LAUNCH((k_multidot2_all<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, cl, total, snew, dvec, c->n, c->ws,
                       c->bstate->dout);
    LBFGSX_HIP(hipGetLastError());
    double r[2 * NC];
    int rc = fetch_doubles(c, 2 * NC, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
    {
        c->bstate->corr_raw[k] = r[k];
        wtd[k] = r[NC + k];
    }
    c->bstate->corr_stash_valid = true;
    return LBFGSX_OK;
}
// the same from the kept compact copy: its positions, then the short list of rows outside it (k_multidot2_wf)
template <class T, int NC>
static int wtd2_wf(lbfgsx_ctx* c, int total, int newest, double* wtd)
{
    lbfgsb_state* b = c->bstate;
    int rc = upload_phys(c);
    if (rc)
        return rc;
    int which[32];
    for (int k = 0; k < total; k++)
        which[k] = k;
    Cols<T, 32> full = col_list<T, 32>(c, which, total);
    Cols<T, 32> wfc = wf_cols<T>(c, total);
    const int fresh_a = newest, fresh_b = c->ncorr + newest;
    const int stand_in = (newest == 0) ? 1 : 0;  // another Y column of the copy: read anyway, so the stale pair costs nothing
    wfc.p[fresh_a] = wfc.p[stand_in];
    wfc.p[fresh_b] = wfc.p[stand_in];
    const T* snew = static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)]));
    const T* ynew = static_cast<const T*>(c->col(c->Y, c->phys[size_t(newest)]));
    const int grid = std::max(1, std::min(std::min(c->grid_for(b->wf_n), b->num_cus), c->ws.maxGrid));
    lbfgsx::poll_arm(c);
    LBFGSX_LAUNCH((k_multidot2_wf<T, NC>), dim3(grid), dim3(kBlock), 0, c->stream, wfc, fresh_a, fresh_b, snew, ynew,
                  static_cast<const T*>(b->dvec), b->wf_idx, b->wf_n, full, b->wtdc_list, int(b->wtdc_n), c->ws, b->dout);
    LBFGSX_HIP(hipGetLastError());
    double r[2 * NC];
    rc = fetch_doubles(c, 2 * NC, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
    {
        b->corr_raw[k] = r[k];
        wtd[k] = r[NC + k];
    }
    b->corr_stash_valid = true;
    b->wtdc_runs++;
    count_wtdc_run();
    return LBFGSX_OK;
}
// the same two passes through the kernels of lbfgsb_x.cuh (any 2c <= 80); outputs packed by 2c
template <class T>
static int wtd2_all_x(lbfgsx_ctx* c, int total, const T* snew, const T* dvec, double* wtd)
{
    lbfgsb_state* b = c->bstate;
    lbfgsx::poll_arm(c);
    int rc = xl::multidot2<T>(c->stream, b->num_cus, colsx_full<T>(c, total), total, snew, dvec, c->n, wsx(c), b->dout);
    if (rc)
        return rc;
    double r[2 * kColsX];
    rc = fetch_doubles(c, 2 * total, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
    {
        b->corr_raw[k] = r[k];
        wtd[k] = r[total + k];
    }
    b->corr_stash_valid = true;
    return LBFGSX_OK;
}
template <class T>
static int wtd2_wf_x(lbfgsx_ctx* c, int total, int newest, double* wtd)
{
    lbfgsb_state* b = c->bstate;
    int rc = upload_phys(c);
    if (rc)
        return rc;
    const ColsX<T> full = colsx_full<T>(c, total);
    ColsX<T> wfc = colsx_wf<T>(c, total);
    const int fresh_a = newest, fresh_b = c->ncorr + newest;
    const int stand_in = (newest == 0) ? 1 : 0;  // another Y column of the copy: read anyway, so the stale pair costs nothing
    wfc.p[fresh_a] = wfc.p[stand_in];
    wfc.p[fresh_b] = wfc.p[stand_in];
    const T* snew = static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)]));
    const T* ynew = static_cast<const T*>(c->col(c->Y, c->phys[size_t(newest)]));
    // the pass also writes the new pair into the copy (lbfgsb_x.cuh: kx_multidot2_wf, dst_a / dst_b): the carried Gram's pass of
    // this iteration's subspace minimisation (lbfgsx_b_gram_pairs_dd) then has nothing to patch.  Remembered by epoch and slot.
    T* dst_a = static_cast<T*>(b->wf) + int64_t(wf_col(c, fresh_a, total)) * b->wf_ld;
    T* dst_b = static_cast<T*>(b->wf) + int64_t(wf_col(c, fresh_b, total)) * b->wf_ld;
    lbfgsx::poll_arm(c);
    rc = xl::multidot2_wf<T>(c->stream, b->num_cus, wfc, total, fresh_a, fresh_b, snew, ynew, static_cast<const T*>(b->dvec), b->wf_idx,
                             b->wf_n, full, b->wtdc_list, int(b->wtdc_n), wsx(c), b->dout, dst_a, dst_b);
    if (rc)
        return rc;
    b->wf_patched_epoch = b->sub_epoch;
    b->wf_patched_slot = newest;
    double r[2 * kColsX];
    rc = fetch_doubles(c, 2 * total, r);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
    {
        b->corr_raw[k] = r[k];
        wtd[k] = r[total + k];
    }
    b->corr_stash_valid = true;
    b->wtdc_runs++;
    count_wtdc_run();
    return LBFGSX_OK;
}
template <class T>
static int cauchy_wtd_t(lbfgsx_ctx* c, double* wtd)
{
    lbfgsb_state* b = c->bstate;
    const int total = 2 * c->ncorr;
    if (b->wtdc_n >= 0 && b->wtdc_n <= int64_t(b->wtdc_cap) && wtdc_ready(c))
    {
        b->corr_defer = false;
        const int newest = (c->ptr + c->m - 1) % c->m;
        if (b->split)
            return wtd2_wf_x<T>(c, total, newest, wtd);
        if (total <= 16)
            return wtd2_wf<T, 16>(c, total, newest, wtd);
        return wtd2_wf<T, 20>(c, total, newest, wtd);
    }
    const bool defer = b->corr_defer;
    b->corr_defer = false;
    if (defer && b->split && total >= 2 && total <= kColsX && !b->multidot_chunked)
    {
        const int newest = (c->ptr + c->m - 1) % c->m;
        const T* snew = static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)]));
        return wtd2_all_x<T>(c, total, snew, static_cast<const T*>(b->dvec), wtd);
    }
    if (defer && total > 8 && total <= 20 && !b->multidot_chunked)
    {
        const int newest = (c->ptr + c->m - 1) % c->m;
        const T* snew = static_cast<const T*>(c->col(c->S, c->phys[size_t(newest)]));
        if (total <= 16)
            return wtd2_all<T, 16>(c, total, snew, static_cast<const T*>(b->dvec), wtd);
        return wtd2_all<T, 20>(c, total, snew, static_cast<const T*>(b->dvec), wtd);
    }
    return wtv_t<T>(c, 0, static_cast<const T*>(b->dvec), 0, wtd, nullptr);
}
int cauchy_wtd(lbfgsx_ctx* c, double* wtd)
{
    int rc = LBFGSX_OK;
    DISPATCH_T(c, { rc = cauchy_wtd_t<T>(c, wtd); });
    return rc;
}
int wtv(lbfgsx_ctx* c, int vsel_id, const void* vcol, int mask, double* out, int64_t* nnz)
{
    int rc = LBFGSX_OK;
    DISPATCH_T(c, { rc = wtv_t<T>(c, vsel_id, static_cast<const T*>(vcol), mask, out, nnz); });
    return rc;
}

#define CB_LAUNCH(M) \
    LBFGSX_LAUNCH((k_wcombine<T, M>), dim3(grid), dim3(kBlock), 0, c->stream, bv, S, Y, c->ld, ph, c->ncorr, cf, has_w, mask, vsel_id, T(theta), c->n, lst, nlst)
template <class T>
static int wcombine_t(lbfgsx_ctx* c, int mode, int mask, int vsel_id, const double* coef, double theta)
{
    // masks inside L u U: walk the index list of the last partition instead of all n rows
    const bool sparse = c->bstate->lu_valid && mask != 0 && (mask & ~(ST_L | ST_U)) == 0;
    const int* lst = sparse ? c->bstate->lu_ptr() : nullptr;
    const int nlst = sparse ? c->bstate->lu_n : 0;
    if (sparse && nlst == 0)
        return LBFGSX_OK;
    const int grid = sparse ? std::max(1, std::min(64, (nlst + kBlock - 1) / kBlock)) : c->grid_for(c->n);
    const int has_w = (coef != nullptr && c->ncorr > 0) ? 1 : 0;
    CoefArg<T> cf;
    for (int k = 0; k < 80; k++)
        cf.c[k] = (has_w && k < 2 * c->ncorr) ? T(coef[k]) : T(0);
    BVecs<T> bv = bvecs<T>(c);
    const T* S = P<T>(c->S);
    const T* Y = P<T>(c->Y);
    const int* ph = c->bstate->phys_dev;
    switch (mode)
    {
    case CB_LINEAR: CB_LAUNCH(CB_LINEAR); break;
    case CB_SOLVE: CB_LAUNCH(CB_SOLVE); break;
    case CB_RHS_ADD: CB_LAUNCH(CB_RHS_ADD); break;
    case CB_LAMBDA: CB_LAUNCH(CB_LAMBDA); break;
    default: CB_LAUNCH(CB_MU); break;
    }
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}
#undef CB_LAUNCH

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_wtv(lbfgsx_ctx* c, int vsel_id, int mask, double* out, int64_t* nnz)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const int64_t na_keep = c->bstate ? c->bstate->na_n : -1;
    int rc = need_bounded(c);
    if (rc)
        return rc;
    // the newly active rows of the Cauchy search that has just ended, listed by its last pass: W_A'(A'd) over the list
    if (mask == ST_NEWACT && na_keep >= 0 && c->bstate->split && 2 * c->ncorr >= 1 && 2 * c->ncorr <= kColsX)
    {
        lbfgsb_state* b = c->bstate;
        const int total = 2 * c->ncorr;
        // the free-set delta the carried Gram asks for next needs nothing from the host: it rides ahead of this pass and its
        // counters are there when this pass's wait returns (contexts that have used the carried form before)
        b->fd_ahead = false;
        if (b->fd_use && b->fprev && free_delta_launch(c) == LBFGSX_OK)
        {
            b->fd_ahead = true;
            b->fd_epoch = b->sub_epoch;
        }
        lbfgsx::poll_arm(c);
        DISPATCH_T(c, {
            rc = xl::list1<T>(c->stream, b->num_cus, colsx_full<T>(c, total), total, bvecs<T>(c), vsel_id, mask, b->na_list, int(na_keep),
                              wsx(c), b->dout);
        });
        if (rc)
            return rc;
        double r[kColsX + 1];
        rc = fetch_doubles(c, total + 1, r);
        if (rc)
            return rc;
        for (int k = 0; k < total; k++)
            out[k] = r[k];
        if (nnz)
            *nnz = int64_t(r[total]);
        return LBFGSX_OK;
    }
    DISPATCH_T(c, { rc = wtv_t<T>(c, vsel_id, static_cast<const T*>(nullptr), mask, out, nnz); });
    return rc;
}

int lbfgsx_b_wtv_lu(lbfgsx_ctx* c, double* out_l, int64_t* nnz_l, double* out_u, int64_t* nnz_u)
{
    return lbfgsx_b_wtv_lu_c(c, out_l, nnz_l, out_u, nnz_u, nullptr);
}

int lbfgsx_b_wtv_lu_c(lbfgsx_ctx* c, double* out_l, int64_t* nnz_l, double* out_u, int64_t* nnz_u, double* negc_dd)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c, false, /*keep_cv=*/true);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    const int total = 2 * c->ncorr;
    if (!b->lu_valid || total < 1 || total > (b->split ? kColsX : 24) || b->multidot_chunked)
    {
        set_error("lbfgsx_b_wtv_lu: needs the index list of L u U and 1 <= 2c <= 80; use lbfgsx_b_wtv per set");
        return LBFGSX_E_INVALID;
    }
    const int nl = b->lu_n;
    const int lgrid = std::max(1, std::min(32, (nl + kBlock - 1) / kBlock));
    int which[kColsX];
    for (int k = 0; k < total; k++)
        which[k] = k;
    double r[2 * (kColsX + 1)];
    int nc = 24;
    // W_{L u U}'(-c) un-rounded (negc_dd; the split-row kernels only): a launch of its own ahead of the pass below, read after
    // the same wait.  What BFGSMatB::solve_PtBP subtracts from W_F'(-c) to have W_P'(-c) without a pass over P.
    bool have_c = false;
    // (round 5) ... or a third set of sums inside the pass below, which walks the same rows (kx_list2<..., WITHC>;
    // LBFGSX_LIST12=0: the launch of its own)
    const bool c_inside = negc_dd && b->split && b->rhs_identity && b->dout_host && b->list12;
    if (c_inside)
        have_c = true;
    else if (negc_dd && b->split && b->rhs_identity && b->dout_host)
    {
        DISPATCH_T(c, {
            const unsigned char* stc = b->cv_live ? bvecs_cv<T>(c).st : static_cast<const unsigned char*>(nullptr);
            const int* stpos = b->cv_live ? b->wf_pos : static_cast<const int*>(nullptr);
            rc = xl::list1<T>(c->stream, b->num_cus, colsx_full<T>(c, total), total, bvecs<T>(c), VS_NEG_CF, ST_L | ST_U, b->lu_ptr(), nl,
                              wsx(c), b->dout + 256, stc, stpos, b->dout + 352);
        });
        if (rc)
            return rc;
        have_c = true;
    }
    // the wait below ends with the last kernel launched before it: the Gram that rides behind this pass, or this pass
    const bool rides = gram_stash_feasible(c, b->lu_ptr(), nl);
    if (!rides)
        lbfgsx::poll_arm(c);
    if (b->split)
    {
        nc = total;  // kx_list2 packs its outputs by 2c: {L dots, nnz_L, U dots, nnz_U}
        DISPATCH_T(c, {
            const unsigned char* stc = b->cv_live ? bvecs_cv<T>(c).st : static_cast<const unsigned char*>(nullptr);
            const int* stpos = b->cv_live ? b->wf_pos : static_cast<const int*>(nullptr);
            rc = xl::list2<T>(c->stream, b->num_cus, colsx_full<T>(c, total), total, bvecs<T>(c), b->lu_ptr(), nl, wsx(c), b->dout, stc,
                              stpos, c_inside ? b->dout + 256 : static_cast<double*>(nullptr),
                              c_inside ? b->dout + 352 : static_cast<double*>(nullptr));
        });
        if (rc)
            return rc;
    }
    else
    DISPATCH_T(c, {
        Cols<T, 32> cl = col_list<T, 32>(c, which, total);
        BVecs<T> bv = bvecs<T>(c);
        // the partition bits of the rows: at their positions while the compact vectors are live
        const unsigned char* stc = b->cv_live ? bvecs_cv<T>(c).st : static_cast<const unsigned char*>(nullptr);
        const int* stpos = b->cv_live ? b->wf_pos : static_cast<const int*>(nullptr);
        if (total <= 8)
        {
            nc = 8;
            LBFGSX_LAUNCH((k_multidot_list2<T, 8>), dim3(lgrid), dim3(kBlock), 0, c->stream, cl, total, bv, b->lu_ptr(), nl, c->ws,
                               b->dout, stc, stpos);
        }
        else if (total <= 16)
        {
            nc = 16;
            LBFGSX_LAUNCH((k_multidot_list2<T, 16>), dim3(lgrid), dim3(kBlock), 0, c->stream, cl, total, bv, b->lu_ptr(), nl,
                               c->ws, b->dout, stc, stpos);
        }
        else
            LBFGSX_LAUNCH((k_multidot_list2<T, 24>), dim3(lgrid), dim3(kBlock), 0, c->stream, cl, total, bv, b->lu_ptr(), nl,
                               c->ws, b->dout, stc, stpos);
    });
    LBFGSX_HIP(hipGetLastError());
    // the solve that follows asks for the Gram over the same rows (the complement identity, lbfgsx_b_gram_fused_dd): it
    // rides behind this pass and is there when this pass's wait returns
    if (rides)
        (void) gram_stash_launch(c, 0, ST_L | ST_U, b->lu_ptr(), nl, /*signal=*/true);
    rc = fetch_doubles(c, 2 * (nc + 1), r);
    gram_stash_settle(c, rc == LBFGSX_OK);
    if (rc)
        return rc;
    for (int k = 0; k < total; k++)
    {
        out_l[k] = r[k];
        out_u[k] = r[nc + 1 + k];
    }
    *nnz_l = int64_t(r[nc]);
    *nnz_u = int64_t(r[2 * nc + 1]);
    if (negc_dd)
    {
        if (have_c)
        {
            const volatile double* h = b->dout_host + 352;
            for (int k = 0; k < 2 * total; k++)
                negc_dd[k] = h[k];
        }
        else
            negc_dd[0] = std::numeric_limits<double>::quiet_NaN();  // not available here: the caller keeps the pass
    }
    return LBFGSX_OK;
}

int lbfgsx_b_wcombine(lbfgsx_ctx* c, int mode, int mask, int vsel_id, const double* coef, double theta)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    if (mode < CB_LINEAR || mode > CB_MU)
    {
        set_error("lbfgsx_b_wcombine: unknown mode");
        return LBFGSX_E_INVALID;
    }
    rc = upload_phys(c);
    if (rc)
        return rc;
    DISPATCH_T(c, { rc = wcombine_t<T>(c, mode, mask, vsel_id, coef, theta); });
    return rc;
}

}  // extern "C"
