// lbfgspp_amd/csrc/lbfgsb_linesearch.hip -- L-BFGS-B device operators around the line search: x = clamp(x), the evaluation, the norms, d'g and
// the largest step (with the first trial ahead), the post statements (with the Cauchy build ahead), the dots of the new pair.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include "lbfgs_kernels.cuh"
#include "launch_args.hpp"

#define LBFGSB_TU "lbfgsb_linesearch"
#include "lbfgsb_state.hpp"

namespace lbfgsx {

template <class T, class OBJ>
static int b_eval_t(lbfgsx_ctx* c, OBJ obj, double* r3)
{
    const BEvalLaunch<T> a = b_eval_launch<T>(c);
    LBFGSX_LAUNCH((k_b_eval<T, OBJ>), dim3(a.grid), dim3(kBlock), 0, c->stream, a.x, a.g, a.lb, a.ub, a.n, obj, a.ws, a.out);
    LBFGSX_HIP(hipGetLastError());
    return fetch_T<T>(c, c->sl.out(0), 3, r3);
}
// the same launch of the kernel compiled for the context's bound term objective
template <class T>
static int b_eval_term_t(lbfgsx_ctx* c, double* r3)
{
    BEvalLaunch<T> a = b_eval_launch<T>(c);
    BoundArgs<T> obj(c);
    void* params[] = {&a.x, &a.g, &a.lb, &a.ub, &a.n, obj.ptr, &a.ws, &a.out};
    int rc = linear_pre_eval<T>(c, obj, a.x);
    if (rc)
        return rc;
    rc = jit_launch(c, JIT_K_B_EVAL, linear_col_grid(c, a.grid), params);
    if (rc)
        return rc;
    return fetch_T<T>(c, c->sl.out(0), 3, r3);
}
template <class T, class OBJ>
static int dg_maxstep_trial_t(lbfgsx_ctx* c, OBJ obj, T step, double* r4)
{
    const DgTrialLaunch<T> a = dg_maxstep_trial_launch<T>(c, step, sizeof(OBJ) >= 2 * sizeof(void*) ? 2 : 0);
    LBFGSX_LAUNCH((k_b_dg_maxstep_trial<T, OBJ>), dim3(a.grid), dim3(kBlock), 0, c->stream, a.xp, a.g0, a.d, a.lb, a.ub, a.step,
                       a.x, a.g, a.n, obj, a.ws, a.out, a.rev);
    LBFGSX_HIP(hipGetLastError());
    return fetch_T<T>(c, c->sl.out(0), 4, r4);
}
template <class T>
static int dg_maxstep_trial_term_t(lbfgsx_ctx* c, T step, double* r4)
{
    DgTrialLaunch<T> a = dg_maxstep_trial_launch<T>(c, step, c->term_np);
    BoundArgs<T> obj(c);
    objective_model_add<T>(c, 2);
    void* params[] = {&a.xp, &a.g0, &a.d, &a.lb, &a.ub, &a.step, &a.x, &a.g, &a.n, obj.ptr, &a.ws, &a.out, &a.rev};
    int rc = linear_pre_trial<T>(c, obj, a.xp, a.d, a.step);
    if (rc)
        return rc;
    rc = jit_launch(c, JIT_K_B_DG_MAXSTEP_TRIAL, linear_col_grid(c, a.grid), params);
    if (rc)
        return rc;
    return fetch_T<T>(c, c->sl.out(0), 4, r4);
}

static std::atomic<int64_t> g_pb_runs{0}, g_pb_hits{0};
void count_pb_hit() { g_pb_hits++; }

}  // namespace lbfgsx

using namespace lbfgsx;

extern "C" {

int lbfgsx_b_force_bounds(lbfgsx_ctx* c)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    return run_force_bounds(c);
}

int lbfgsx_b_force_bounds_deferred(lbfgsx_ctx* c)
{
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const char* e = getenv("LBFGSX_FORCE_FUSE");  // =0: A/B, run the statement as its own pass
    if (e && e[0] == '0')
        return lbfgsx_b_force_bounds(c);
    c->bstate->force_pending = true;
    return LBFGSX_OK;
}

int lbfgsx_b_eval(lbfgsx_ctx* c, int objective, double* fx, double* projgnorm, double* xnorm2)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    double r[3];
    rc = LBFGSX_E_INVALID;
    DISPATCH_T(c, {
        if (objective == LBFGSX_OBJ_DIAG_QUAD)
            rc = b_eval_t<T>(c, ObjQuad<T>{P<T>(c->a), P<T>(c->b)}, r);
        else if (objective == LBFGSX_OBJ_EXT_ROSENBROCK)
            rc = b_eval_t<T>(c, ObjRosen<T>{}, r);
        else if (lbfgsx::term_bound(c, objective))
            rc = b_eval_term_t<T>(c, r);
        else
            set_error("lbfgsx_b_eval: unknown objective");
    });
    if (rc)
        return rc;
    if (fx) *fx = r[0];
    if (xnorm2) *xnorm2 = r[1];
    if (projgnorm) *projgnorm = r[2];
    return LBFGSX_OK;
}

int lbfgsx_b_norms(lbfgsx_ctx* c, double* projgnorm, double* xnorm2)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[2];
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_b_norms<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->xb[c->cur]), P<T>(c->gb[c->cur]),
                           P<T>(c->lb), P<T>(c->ub), c->n, c->ws, c->out_slot<T>());
        LBFGSX_HIP(hipGetLastError());
        rc = fetch_T<T>(c, c->sl.out(0), 2, r);
    });
    if (rc)
        return rc;
    if (xnorm2) *xnorm2 = r[0];
    if (projgnorm) *projgnorm = r[1];
    return LBFGSX_OK;
}

int lbfgsx_b_dg_maxstep(lbfgsx_ctx* c, double* dg, double* step_max)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[2];
    DISPATCH_T(c, {
        lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(c->n) * 5 * sizeof(T));  // byte model: x, g, d, lb, ub
        LBFGSX_LAUNCH((k_b_dg_maxstep<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->xb[c->cur]),
                           P<T>(c->gb[c->cur]), P<T>(c->d), P<T>(c->lb), P<T>(c->ub), c->n, c->ws, c->out_slot<T>());
        LBFGSX_HIP(hipGetLastError());
        rc = fetch_T<T>(c, c->sl.out(0), 2, r);
    });
    if (rc)
        return rc;
    if (dg) *dg = r[0];
    if (step_max) *step_max = r[1];
    return LBFGSX_OK;
}

int lbfgsx_b_dg_maxstep_trial(lbfgsx_ctx* c, int objective, double step0, double* dg, double* step_max)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const bool use = c->bstate && c->bstate->st_use;
    const bool builtin = objective == LBFGSX_OBJ_DIAG_QUAD || objective == LBFGSX_OBJ_EXT_ROSENBROCK || lbfgsx::term_bound(c, objective);
    // after a trial that was evaluated ahead and not used (step_max < 1: the early iterations) a few iterations go without
    if (!use || !builtin || !c->outmap_dev || c->xp != c->cur || !(step0 > 0.0) || c->st_cooldown > 0)
    {
        if (c->st_cooldown > 0)
            c->st_cooldown--;
        return lbfgsx_b_dg_maxstep(c, dg, step_max);
    }
    int rc = need_bounded(c);
    if (rc)
        return rc;
    double r[4];
    rc = LBFGSX_E_INVALID;
    DISPATCH_T(c, {
        if (objective == LBFGSX_OBJ_DIAG_QUAD)
            rc = dg_maxstep_trial_t<T>(c, ObjQuad<T>{P<T>(c->a), P<T>(c->b)}, T(step0), r);
        else if (objective == LBFGSX_OBJ_EXT_ROSENBROCK)
            rc = dg_maxstep_trial_t<T>(c, ObjRosen<T>{}, T(step0), r);
        else
            rc = dg_maxstep_trial_term_t<T>(c, T(step0), r);
    });
    if (rc)
        return rc;
    c->st_valid = true;
    c->st_obj = objective;
    c->st_xp = c->xp;
    c->st_trial = c->trial;
    c->st_step = step0;
    c->st_f = r[2];
    c->st_dg = r[3];
    c->st_runs++;
    if (dg) *dg = r[0];
    if (step_max) *step_max = r[1];
    return LBFGSX_OK;
}

int lbfgsx_b_trial_ahead_counts(const lbfgsx_ctx* c, int64_t out[2])
{
    if (!c || !out)
        return LBFGSX_E_INVALID;
    out[0] = c->st_runs;
    out[1] = c->st_hits;
    return LBFGSX_OK;
}

int lbfgsx_b_post_linesearch(lbfgsx_ctx* c, double* projgnorm, double* xnorm2, double* sy, double* yy)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[4];
    // exact max |s|, max |y| of the new column pair ride along (the fixed-point scale of the integer Gram, gram_i8.cuh)
    unsigned long long* cmx = nullptr;
    if (c->bstate->gram_i8)
    {
        cmx = c->bstate->colmax + 2 * size_t(c->spare);
        LBFGSX_HIP(hipMemsetAsync(cmx, 0, 2 * sizeof(unsigned long long), c->stream));
        c->bstate->colmax_ok[size_t(c->spare)] = 1;
    }
    DISPATCH_T(c, {
        lbfgsx::poll_arm(c);
        lbfgsx::model_add(double(c->n) * 8 * sizeof(T));  // byte model: x, xp, g, gp, lb, ub read, s and y written
        LBFGSX_LAUNCH((k_b_post<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->xb[c->cur]), P<T>(c->xb[c->xp]),
                           P<T>(c->gb[c->cur]), P<T>(c->gb[c->xp]), P<T>(c->lb), P<T>(c->ub), P<T>(c->col(c->S, c->spare)),
                           P<T>(c->col(c->Y, c->spare)), c->n, c->ws, c->out_slot<T>(),
                           P<T>(c->sc) + c->sl.ys(c->spare), P<T>(c->sc) + c->sl.theta(c->spare), cmx);
        LBFGSX_HIP(hipGetLastError());
        rc = fetch_T<T>(c, c->sl.out(0), 4, r);
    });
    if (rc)
        return rc;
    c->pend_sy = r[1];
    c->pend_yy = r[2];
    c->pending = true;
    if (xnorm2) *xnorm2 = r[0];
    if (sy) *sy = r[1];
    if (yy) *yy = r[2];
    if (projgnorm) *projgnorm = r[3];
    return LBFGSX_OK;
}

int lbfgsx_b_post_build_counts(int64_t out[2], int reset)
{
    if (out)
    {
        out[0] = g_pb_runs.load();
        out[1] = g_pb_hits.load();
    }
    if (reset)
        g_pb_runs = g_pb_hits = 0;
    return LBFGSX_OK;
}

int lbfgsx_b_post_linesearch_build(lbfgsx_ctx* c, double tau, double* projgnorm, double* xnorm2, double* sy, double* yy)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    lbfgsb_state* b = c->bstate;
    b->pb_valid = false;
    // One wait has to serve both halves (mapped outputs); the integer Gram wants the column maxima of k_b_post; a partial
    // sort whose selection rides behind the build keeps the two-pass form.  The build half is computed for the state the
    // solver will be in if it goes on and accepts the pair: lbfgsx_b_cauchy_build_partial checks that it is.
    const bool tau_ok = tau > 0.0 && std::isfinite(tau);
    const bool sel_inline = tau_ok && b->psel_use && b->psel_last >= 0 && b->psel_last <= lbfgsb_state::kPselMax &&
                            c->n < (int64_t(1) << 31) && psel_alloc(c);
    const bool sel_ahead = !sel_inline && b->stash_use && b->dout_host && tau_ok;
    if (!(b->pb_use && c->outmap_dev && b->dout_host && !b->gram_i8 && !sel_ahead))
        return lbfgsx_b_post_linesearch(c, projgnorm, xnorm2, sy, yy);
    const int grid = c->grid_for(c->n);
    double r[4];
    DISPATCH_T(c, {
        BVecs<T> bv = bvecs<T>(c);
        const bool wc = wtdc_ready(c, true) && wtdc_alloc(c);
        lbfgsx::poll_arm(c);
        // the sort keys over all n rows are only wanted when the candidates of the partial sort are NOT listed by this pass; the
        // indices once (ensure_keys rebuilds either on demand)
        T* keys_arg = sel_inline ? static_cast<T*>(nullptr) : P<T>(b->keys_in);
        int* vals_arg = b->vals_iota ? static_cast<int*>(nullptr) : b->vals_in;
        // byte model: x, xp, g, gp, lb, ub and the positions read; s, y, brk, d, xcp (and the keys / indices, when wanted) written
        lbfgsx::model_add(double(c->n) * (11 * sizeof(T) + 4 + (keys_arg ? sizeof(T) : 0) + (vals_arg ? 4 : 0)));
        b->keys_valid = keys_arg != nullptr;
        if (vals_arg)
            b->vals_iota = true;
        LBFGSX_LAUNCH((k_b_post_build<T>), dim3(grid), dim3(kBlock), 0, c->stream, bv, P<T>(c->xb[c->xp]), P<T>(c->gb[c->xp]),
                           P<T>(c->col(c->S, c->spare)), P<T>(c->col(c->Y, c->spare)), c->out_slot<T>(),
                           P<T>(c->sc) + c->sl.ys(c->spare), P<T>(c->sc) + c->sl.theta(c->spare), keys_arg, vals_arg,
                           c->n, c->ws, b->dout, wc ? b->wf_pos : static_cast<const int*>(nullptr), b->wtdc_list, b->wtdc_cnt,
                           b->wtdc_cap, T(tau), sel_inline ? b->psel_list : static_cast<int*>(nullptr), b->psel_cnt, b->psel_cap);
        LBFGSX_HIP(hipGetLastError());
        rc = fetch_T<T>(c, c->sl.out(0), 4, r);
        if (rc)
            return rc;
        const volatile double* h = b->dout_host;  // same completion word: the build half's numbers have arrived, too
        for (int i = 0; i < 6; i++)
            b->pb_r[i] = h[i];
        b->pb_wc = wc;
    });
    b->pb_valid = true;
    b->pb_cur = c->cur;
    b->pb_writes = c->vec_writes;
    b->pb_tau = tau;
    b->pb_sel_inline = sel_inline;
    g_pb_runs++;
    c->pend_sy = r[1];
    c->pend_yy = r[2];
    c->pending = true;
    if (xnorm2) *xnorm2 = r[0];
    if (sy) *sy = r[1];
    if (yy) *yy = r[2];
    if (projgnorm) *projgnorm = r[3];
    return LBFGSX_OK;
}

int lbfgsx_b_correction_dots_defer(lbfgsx_ctx* c)
{
    int rc = need_bounded(c);
    if (rc)
        return rc;
    c->bstate->corr_defer = c->ncorr > 0;
    c->bstate->corr_stash_valid = false;
    return LBFGSX_OK;
}

int lbfgsx_b_correction_dots(lbfgsx_ctx* c, double* sdots, double* ydots)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    if (c->ncorr < 1)
        return LBFGSX_OK;
    const int newest = (c->ptr + c->m - 1) % c->m;  // slot written by the last commit (BFGSMat.h:83,97)
    double raw[80];
    c->bstate->corr_defer = false;
    if (c->bstate->corr_stash_valid)  // delivered by the W'd pass of lbfgsx_b_cauchy_build* (k_multidot2_all)
    {
        c->bstate->corr_stash_valid = false;
        for (int j = 0; j < c->ncorr; j++)
        {
            ydots[j] = c->bstate->corr_raw[j];
            sdots[j] = c->bstate->corr_raw[c->ncorr + j];
        }
        return LBFGSX_OK;
    }
    rc = wtv(c, 0, c->col(c->S, c->phys[size_t(newest)]), 0, raw, nullptr);  // v = the newest s
    if (rc)
        return rc;
    for (int j = 0; j < c->ncorr; j++)
    {
        ydots[j] = raw[j];
        sdots[j] = raw[c->ncorr + j];
    }
    return LBFGSX_OK;
}

int lbfgsx_b_dot_drt_g(lbfgsx_ctx* c, double* dg)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    const int grid = c->grid_for(c->n);
    double r[2];
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_dot<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->d), P<T>(c->gb[c->cur]),
                           static_cast<const T*>(nullptr), c->n, c->ws, c->out_slot<T>());
        LBFGSX_HIP(hipGetLastError());
        int rc = fetch_T<T>(c, c->sl.out(0), 1, r);
        if (rc)
            return rc;
    });
    *dg = r[0];
    return LBFGSX_OK;
}

int lbfgsx_b_dir_from_xcp(lbfgsx_ctx* c, int normalize)
{
    lbfgsx::DeviceGuard dev_guard_(c->device);
    int rc = need_bounded(c);
    if (rc)
        return rc;
    const int grid = c->grid_for(c->n);
    double r[1];
    DISPATCH_T(c, {
        LBFGSX_LAUNCH((k_b_dir_from_xcp<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->xcp), P<T>(c->xb[c->cur]),
                           P<T>(c->d), c->n, c->ws, c->out_slot<T>());
        LBFGSX_HIP(hipGetLastError());
        if (normalize)
        {
            rc = fetch_T<T>(c, c->sl.out(0), 1, r);
            if (rc)
                return rc;
            const T z = T(r[0]);
            if (z > T(0))  // Eigen normalize(): divide only when the squared norm is positive
                LBFGSX_LAUNCH((k_b_scale_div<T>), dim3(grid), dim3(kBlock), 0, c->stream, P<T>(c->d), T(std::sqrt(z)), c->n);
        }
    });
    LBFGSX_HIP(hipGetLastError());
    return LBFGSX_OK;
}

}  // extern "C"
