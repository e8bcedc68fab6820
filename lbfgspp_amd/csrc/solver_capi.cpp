// lbfgspp_amd/csrc/solver_capi.cpp -- liblbfgsx_solver.so: the drop-in C++ solver templates instantiated
// for the built-in objectives, for a term objective compiled at run time and for a C callback on device memory behind
// include/lbfgsx_solver.h.  Plain host C++ (g++),
// links liblbfgsx.so.
#include <cstdio>
#include <cstring>
#include <atomic>
#include <memory>
#include <thread>

#include "../../include/LBFGS.h"
#include "../../include/LBFGSB.h"
#include "../../include/LBFGSBatched.h"
#include "../../include/lbfgsx_solver.h"
#include "form_table.hpp"

using namespace LBFGSpp;

struct lbfgsx_solver
{
    virtual ~lbfgsx_solver() {}
    virtual void prepare(int64_t n) = 0;
    virtual lbfgsx_ctx* ctx() = 0;
    virtual void set_hook(void (*fn)(int, void*), void* user) = 0;
    virtual int hessians(double*, double*) { return LBFGSX_E_INVALID; }
    virtual int set_recursion(int) { return LBFGSX_E_INVALID; }
    virtual int set_direction_scale(double) { return LBFGSX_E_INVALID; }
    virtual int set_allreduce(void (*)(double*, int, void*), void*) { return LBFGSX_E_INVALID; }
    virtual int set_devices(const int*, int) { return LBFGSX_E_INVALID; }
    int dtype = LBFGSX_F64;
    long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long stats_submin_us = 0;
    long long stats2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long stats3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    virtual void minimize(int objective, int64_t n, const void* a, const void* b, void* x, const void* lb,
                          const void* ub, lbfgsx_trace* tr, lbfgsx_result* out) = 0;
    virtual void minimize_fn(int64_t n, lbfgsx_objective_fn fn, void* user, void* x, const void* lb, const void* ub,
                             lbfgsx_trace* tr, lbfgsx_result* out) = 0;
    // what minimize_obj is asked for beside the handle: the form of the entry point that was called (LBFGSX_FORM_TERM: the one
    // for a term or chain objective; LBFGSX_FORM_LINEAR: the one for either linear form) and that form's own arguments
    struct ObjSpec
    {
        int form = LBFGSX_FORM_TERM;
        // a lattice form's extents (slabs: three axes) and mask (a form that has one)
        int64_t slabs = 0, rows = 0, cols = 0;
        int periodic = 0;
        // the edges of a graph objective, and the element counts of the host data arrays of a form with a list (null: n
        // each); elems: the connectivity table of a mesh objective (E rows) in place of ei and ej
        int64_t E = 0;
        const int32_t *ei = nullptr, *ej = nullptr;
        int on_device = 0;
        const int64_t* counts = nullptr;
        const int32_t* elems = nullptr;
        // a linear-model objective's CSR matrix: R rows, nnz entries
        int64_t R = 0, nnz = 0;
        const int32_t *rowptr = nullptr, *col = nullptr;
        const void* val = nullptr;
        int lanes = 0;
        // a graph-regularised linear-model objective has both: the matrix above and the edges ei, ej, which are device arrays
        // when edges_dev says so (on_device then speaks of the matrix alone)
        int edges_dev = 0;
        // a dense linear-model objective's matrix: R rows, row stride lda
        const void* A = nullptr;
        int64_t lda = 0;
    };
    virtual void minimize_obj(const lbfgsx_objective* obj, int64_t n, const ObjSpec& spec, const void* const p[4], int host_mask,
                              const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* tr, lbfgsx_result* out) = 0;
};

namespace {

template <class Scalar, class P>
void fill_common(P& q, const lbfgsx_params* p)
{
    q.m = p->m;
    q.epsilon = Scalar(p->epsilon);
    q.epsilon_rel = Scalar(p->epsilon_rel);
    q.past = p->past;
    q.delta = Scalar(p->delta);
    q.max_iterations = p->max_iterations;
    q.max_linesearch = p->max_linesearch;
    q.min_step = Scalar(p->min_step);
    q.max_step = Scalar(p->max_step);
    q.ftol = Scalar(p->ftol);
    q.wolfe = Scalar(p->wolfe);
}

template <class Scalar>
struct HostSpan  // minimal "vector" over caller memory for minimize(f, x, fx)
{
    Scalar* p;
    int64_t n;
    Scalar* data() { return p; }
    const Scalar* data() const { return p; }
    int64_t size() const { return n; }
    void resize(int64_t) {}
};

template <class Scalar>
void install_trace(lbfgsx_trace* tr, std::function<void(int, Scalar, DeviceState<Scalar>&)>& cb)
{
    if (!tr)
    {
        cb = nullptr;
        return;
    }
    tr->count = 0;
    cb = [tr](int k, Scalar fx, DeviceState<Scalar>& st) {
        if (k >= tr->cap)
            return;
        tr->fx[k] = double(fx);
        if (tr->xs)
        {
            // the point just evaluated: the trial buffer, or X for the very first evaluation
            const int which = (k == 0) ? LBFGSX_VEC_X : LBFGSX_VEC_XT;
            detail::check(lbfgsx_gather(st.ctx(), which, tr->stride, tr->xs + int64_t(k) * tr->nsamp));
        }
        tr->count = k + 1;
    };
}

// lbfgsx_objective_fn as the device functor the solver templates take (LBFGSpp/Device.h: it names DeviceVector)
template <class Scalar>
struct CallbackObjective
{
    lbfgsx_objective_fn fn;
    void* user;
    int calls = 0;
    Scalar operator()(const DeviceVector<Scalar>& x, DeviceVector<Scalar>& grad)
    {
        double fx = 0.0;
        calls++;
        const int rc = fn(user, x.data(), grad.data(), x.size(), &fx);
        if (rc != 0)
            throw UserAbort("the objective callback returned " + std::to_string(rc) + " at evaluation " + std::to_string(calls));
        return Scalar(fx);
    }
};

// a compiled term objective with its data (device pointers, or host arrays where host_mask has the slot's bit) and scalars
template <class Scalar>
void fill_term(TermObjective<Scalar>& f, const void* const p[4], int host_mask, const double c[8],
               const int64_t* counts = nullptr)
{
    const Scalar* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++)
    {
        const Scalar* q = p ? static_cast<const Scalar*>(p[k]) : nullptr;
        if (q && (host_mask >> k & 1) && counts && counts[k] > 0)
            f.host_data(k, q, counts[k]);
        else if (q && (host_mask >> k & 1))
            f.host_data(k, q);
        else
            dev[k] = q;
    }
    f.data(dev[0], dev[1], dev[2], dev[3]);
    if (c)
        f.scalars(c, 8);
}

// the one objective object the spec asks for -- the class of the entry point's form around the handle, with the form's
// arguments -- filled with its data and handed to run.  The class is chosen by the entry point that was called, never by the
// handle: a handle of another form is refused by that class's bind call
template <class Scalar, class Run>
void with_objective(const lbfgsx_objective* obj, const lbfgsx_solver::ObjSpec& s, const void* const p[4], int host_mask,
                    const double c[8], Run&& run)
{
    const auto go = [&](TermObjective<Scalar>& f) {
        fill_term<Scalar>(f, p, host_mask, c, s.counts);
        run(f);
    };
    const Scalar* val = static_cast<const Scalar*>(s.val);
    switch (s.form)
    {
    case LBFGSX_FORM_GRID: { GridObjective<Scalar> f(obj, s.rows, s.cols); return go(f); }
    case LBFGSX_FORM_VOLUME: { VolumeObjective<Scalar> f(obj, s.slabs, s.rows, s.cols); return go(f); }
    case LBFGSX_FORM_GRID_PERIODIC: { PeriodicGridObjective<Scalar> f(obj, s.rows, s.cols, s.periodic); return go(f); }
    case LBFGSX_FORM_VOLUME_PERIODIC: { PeriodicVolumeObjective<Scalar> f(obj, s.slabs, s.rows, s.cols, s.periodic); return go(f); }
    case LBFGSX_FORM_GRID_FIELD: { GridFieldObjective<Scalar> f(obj, s.rows, s.cols, s.periodic); return go(f); }
    case LBFGSX_FORM_GRID_STENCIL: { StencilObjective<Scalar> f(obj, s.rows, s.cols, s.periodic); return go(f); }
    case LBFGSX_FORM_GRAPH: { GraphObjective<Scalar> f(obj); f.edges(s.E, s.ei, s.ej, s.on_device != 0); return go(f); }
    case LBFGSX_FORM_MESH: { MeshObjective<Scalar> f(obj); f.elements(s.E, s.elems, s.on_device != 0); return go(f); }
    case LBFGSX_FORM_LINEAR: {  // either linear form: lbfgsx_objective_bind_linear takes both
        LinearObjective<Scalar> f(obj);
        f.matrix(s.R, s.nnz, s.rowptr, s.col, val, s.on_device != 0, s.lanes);
        return go(f);
    }
    case LBFGSX_FORM_LINEAR_GRAPH: {
        GraphLinearObjective<Scalar> f(obj);
        f.matrix(s.R, s.nnz, s.rowptr, s.col, val, s.on_device != 0, s.lanes).edges(s.E, s.ei, s.ej, s.edges_dev != 0);
        return go(f);
    }
    case LBFGSX_FORM_DENSE: {
        DenseLinearObjective<Scalar> f(obj);
        f.matrix(s.R, static_cast<const Scalar*>(s.A), s.lda, s.on_device != 0, s.lanes);
        return go(f);
    }
    default: { TermObjective<Scalar> f(obj); return go(f); }  // a term or chain objective: bound without arguments
    }
}

template <class Scalar, template <class> class LS>
struct LbfgsImpl : lbfgsx_solver
{
    LBFGSParam<Scalar> param;
    std::unique_ptr<LBFGSSolver<Scalar, LS> > solver;
    LbfgsImpl(const lbfgsx_params* p, int device)
    {
        fill_common<Scalar>(param, p);
        param.linesearch = p->linesearch;
        solver.reset(new LBFGSSolver<Scalar, LS>(param));
        solver->set_device(device);
    }
    void prepare(int64_t n) override { solver->prepare_resident(n); }
    lbfgsx_ctx* ctx() override { return solver->device_state().ctx(); }
    void set_hook(void (*fn)(int, void*), void* user) override
    {
        if (fn)
            solver->set_iteration_hook([fn, user](int k) { fn(k, user); });
        else
            solver->set_iteration_hook(nullptr);
    }
    int set_recursion(int form) override
    {
        if (form != RECURSION_VECTOR && form != RECURSION_GRAM_SPACE &&
            !(form == RECURSION_GRAM_SPACE_F32H && std::is_same<Scalar, double>::value))
            return LBFGSX_E_INVALID;
        solver->set_recursion(form);
        return LBFGSX_OK;
    }
    int set_direction_scale(double a) override
    {
        solver->set_direction_scale(a);
        return LBFGSX_OK;
    }
    int set_allreduce(void (*fn)(double*, int, void*), void* user) override
    {
        if (fn)
            solver->set_reducer([fn, user](double* v, int k) { fn(v, k, user); });
        else
            solver->set_reducer(nullptr);
        return LBFGSX_OK;
    }
    int set_devices(const int* devs, int ndev) override
    {
        solver->set_devices(devs && ndev > 0 ? std::vector<int>(devs, devs + ndev) : std::vector<int>());
        return LBFGSX_OK;
    }
    int hessians(double* B, double* H) override
    {
        const auto mb = solver->final_approx_hessian();
        const auto mh = solver->final_approx_inverse_hessian();
        const int n = mb.rows();
        for (int j = 0; j < n; j++)
            for (int i = 0; i < n; i++)
            {
                B[size_t(j) * size_t(n) + size_t(i)] = double(mb(i, j));
                H[size_t(j) * size_t(n) + size_t(i)] = double(mh(i, j));
            }
        return LBFGSX_OK;
    }
    void minimize(int objective, int64_t n, const void* a, const void* b, void* x, const void*, const void*,
                  lbfgsx_trace* tr, lbfgsx_result* out) override
    {
        BuiltinObjective<Scalar> f(objective, static_cast<const Scalar*>(a), static_cast<const Scalar*>(b));
        run(f, n, x, tr, out);
    }
    void minimize_fn(int64_t n, lbfgsx_objective_fn fn, void* user, void* x, const void*, const void*, lbfgsx_trace* tr,
                     lbfgsx_result* out) override
    {
        CallbackObjective<Scalar> f = {fn, user};
        try
        {
            run(f, n, x, tr, out);
        }
        catch (const UserAbort&)
        {
            out->nfev = f.calls;  // the failing call included
            throw;
        }
    }
    void minimize_obj(const lbfgsx_objective* obj, int64_t n, const ObjSpec& spec, const void* const p[4], int host_mask,
                      const double c[8], void* x, const void*, const void*, lbfgsx_trace* tr, lbfgsx_result* out) override
    {
        with_objective<Scalar>(obj, spec, p, host_mask, c, [&](TermObjective<Scalar>& f) { run(f, n, x, tr, out); });
    }
    template <class Foo>
    void run(Foo& f, int64_t n, void* x, lbfgsx_trace* tr, lbfgsx_result* out)
    {
        std::function<void(int, Scalar, DeviceState<Scalar>&)> cb;
        install_trace<Scalar>(tr, cb);
        solver->set_trace(cb);
        Scalar fx = Scalar(0);
        try
        {
            if (x)
            {
                HostSpan<Scalar> xv = {static_cast<Scalar*>(x), n};
                out->niter = solver->minimize(f, xv, fx);
            }
            else
                out->niter = solver->minimize_resident(f, n, fx);
        }
        catch (...)
        {
            out->nfev = solver->num_evaluations();
            throw;
        }
        out->fx = double(fx);
        out->gnorm = double(solver->final_grad_norm());
        out->nfev = solver->num_evaluations();
    }
};

template <class Scalar>
struct LbfgsbImpl : lbfgsx_solver
{
    LBFGSBParam<Scalar> param;
    std::unique_ptr<LBFGSBSolver<Scalar> > solver;
    LbfgsbImpl(const lbfgsx_params* p, int device)
    {
        fill_common<Scalar>(param, p);
        param.max_submin = p->max_submin;
        solver.reset(new LBFGSBSolver<Scalar>(param));
        solver->set_device(device);
    }
    void prepare(int64_t n) override { solver->prepare_resident(n); }
    lbfgsx_ctx* ctx() override { return solver->device_state().ctx(); }
    // the solver's statistics as lbfgsx_solver_stats* serve them: refreshed at the end of minimize() and before every call of
    // the iteration hook, so that a hook can difference them per iteration (bench.py: the sweeps, sorted break points and
    // launches of the SAME iterations it times)
    void publish_stats()
    {
        const auto& st = solver->stats();
        stats[0] = st.gcp_crossings;
        stats[1] = st.submin_sweeps;
        stats[2] = st.submin_calls;
        stats[3] = st.submin_unconverged;
        stats[4] = st.resets;
        stats[5] = (long long) (st.gcp_build_s * 1e6);
        stats[6] = (long long) (st.gcp_fetch_s * 1e6);
        stats[7] = (long long) (st.gcp_total_s * 1e6);
        stats_submin_us = (long long) (st.submin_s * 1e6);
        stats2[0] = st.gcp_dev_crossings;
        stats2[1] = st.gcp_sort_fallbacks;
        stats2[2] = st.gcp_partial_sorts;
        stats2[3] = (long long) (st.submin_s * 1e6);
        stats2[4] = (long long) (st.linesearch_s * 1e6);
        stats2[5] = (long long) (st.correction_s * 1e6);
        stats2[6] = st.submin_fused_sweeps;
        stats2[7] = st.gram_carried;
        stats3[0] = st.gcp_searches;
        stats3[1] = st.gcp_nord;
        stats3[2] = st.gcp_sorted;
        stats3[3] = st.rhs_identities;
    }
    void set_hook(void (*fn)(int, void*), void* user) override
    {
        if (fn)
            solver->set_iteration_hook([this, fn, user](int k) {
                publish_stats();
                fn(k, user);
            });
        else
            solver->set_iteration_hook(nullptr);
    }
    void minimize(int objective, int64_t n, const void* a, const void* b, void* x, const void* lb, const void* ub,
                  lbfgsx_trace* tr, lbfgsx_result* out) override
    {
        BuiltinObjective<Scalar> f(objective, static_cast<const Scalar*>(a), static_cast<const Scalar*>(b));
        run(f, n, x, lb, ub, tr, out);
    }
    void minimize_fn(int64_t n, lbfgsx_objective_fn fn, void* user, void* x, const void* lb, const void* ub, lbfgsx_trace* tr,
                     lbfgsx_result* out) override
    {
        CallbackObjective<Scalar> f = {fn, user};
        try
        {
            run(f, n, x, lb, ub, tr, out);
        }
        catch (const UserAbort&)
        {
            out->nfev = f.calls;  // the failing call included
            throw;
        }
    }
    void minimize_obj(const lbfgsx_objective* obj, int64_t n, const ObjSpec& spec, const void* const p[4], int host_mask,
                      const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* tr, lbfgsx_result* out) override
    {
        with_objective<Scalar>(obj, spec, p, host_mask, c, [&](TermObjective<Scalar>& f) { run(f, n, x, lb, ub, tr, out); });
    }
    template <class Foo>
    void run(Foo& f, int64_t n, void* x, const void* lb, const void* ub, lbfgsx_trace* tr, lbfgsx_result* out)
    {
        std::function<void(int, Scalar, DeviceState<Scalar>&)> cb;
        install_trace<Scalar>(tr, cb);
        solver->set_trace(cb);
        Scalar fx = Scalar(0);
        try
        {
            if (x)
            {
                if (!lb || !ub)
                    throw std::invalid_argument("'lb' and 'ub' must have the same size as 'x'");
                HostSpan<Scalar> xv = {static_cast<Scalar*>(x), n};
                const HostSpan<Scalar> lv = {const_cast<Scalar*>(static_cast<const Scalar*>(lb)), n};
                const HostSpan<Scalar> uv = {const_cast<Scalar*>(static_cast<const Scalar*>(ub)), n};
                out->niter = solver->minimize(f, xv, fx, lv, uv);
            }
            else
                out->niter = solver->minimize_resident(f, n, fx);
        }
        catch (...)
        {
            out->nfev = solver->num_evaluations();
            throw;
        }
        out->fx = double(fx);
        out->gnorm = double(solver->final_grad_norm());
        out->nfev = solver->num_evaluations();
        publish_stats();
    }
};

template <class Scalar>
lbfgsx_solver* make_lbfgs(int ls, const lbfgsx_params* p, int device)
{
    switch (ls)
    {
    case LBFGSX_LS_NOCEDAL_WRIGHT: return new LbfgsImpl<Scalar, LineSearchNocedalWright>(p, device);
    case LBFGSX_LS_MORE_THUENTE: return new LbfgsImpl<Scalar, LineSearchMoreThuente>(p, device);
    case LBFGSX_LS_BACKTRACKING: return new LbfgsImpl<Scalar, LineSearchBacktracking>(p, device);
    case LBFGSX_LS_BRACKETING: return new LbfgsImpl<Scalar, LineSearchBracketing>(p, device);
    default: throw std::invalid_argument("unknown line search");
    }
}

template <class F>
int guarded(lbfgsx_result* out, F&& body)
{
    int status = 0;
    std::string keep;
    try
    {
        body();
    }
    catch (const UserAbort& e)
    {
        status = LBFGSX_E_USER;
        keep = e.what();
    }
    catch (const std::invalid_argument& e)
    {
        status = LBFGSX_E_INVALID;
        keep = e.what();
    }
    catch (const std::logic_error& e)
    {
        status = LBFGSX_E_LOGIC;
        keep = e.what();
    }
    catch (const std::exception& e)
    {
        status = LBFGSX_E_RUNTIME;
        keep = e.what();
    }
    if (out)
    {
        out->status = status;
        std::snprintf(out->msg, sizeof(out->msg), "%s", keep.c_str());
    }
    return status;
}

thread_local lbfgsx_result g_create_result;

}  // namespace

extern "C" {

int lbfgsx_solver_create(lbfgsx_solver** out, int algo, int dtype, int linesearch, const lbfgsx_params* p, int device)
{
    *out = nullptr;
    return guarded(&g_create_result, [&]() {
        if (dtype != LBFGSX_F64 && dtype != LBFGSX_F32)
            throw std::invalid_argument("unknown dtype");
        if (algo == LBFGSX_ALGO_LBFGS)
            *out = (dtype == LBFGSX_F64) ? make_lbfgs<double>(linesearch, p, device) : make_lbfgs<float>(linesearch, p, device);
        else if (algo == LBFGSX_ALGO_LBFGSB)
        {
            if (linesearch != LBFGSX_LS_MORE_THUENTE)
                throw std::invalid_argument("LBFGSBSolver is instantiated with LineSearchMoreThuente only");
            *out = (dtype == LBFGSX_F64) ? static_cast<lbfgsx_solver*>(new LbfgsbImpl<double>(p, device))
                                         : static_cast<lbfgsx_solver*>(new LbfgsbImpl<float>(p, device));
        }
        else
            throw std::invalid_argument("unknown algorithm");
        (*out)->dtype = dtype;
    });
}

const char* lbfgsx_solver_create_error(void) { return g_create_result.msg; }

void lbfgsx_solver_destroy(lbfgsx_solver* s) { delete s; }

int lbfgsx_solver_prepare(lbfgsx_solver* s, int64_t n)
{
    lbfgsx_result r;
    return guarded(&r, [&]() { s->prepare(n); });
}

lbfgsx_ctx* lbfgsx_solver_ctx(lbfgsx_solver* s) { return s->ctx(); }

// Test entry: feed `npairs` corrections into a fresh L-BFGS-B matrix, then run Cauchy::get_cauchy_point and
// SubspaceMin::subspace_minimize of the drop-in headers at (x0, g, lb, ub).  Outputs are host arrays.
int lbfgsx_test_cauchy_subspace(int dtype, int64_t n, int m, int npairs, const void* S, const void* Y, const void* x0,
                                const void* g, const void* lb, const void* ub, int max_submin, void* xcp, double* vecc,
                                unsigned char* state, void* drt, long long counts[4], char* errbuf, int errlen)
{
    lbfgsx_result r;
    int rc = guarded(&r, [&]() {
        auto body = [&](auto tag) {
            typedef decltype(tag) T;
            DeviceState<T> dev;
            dev.ensure(n, m, LBFGSX_FLAG_BOUNDED, 0);
            lbfgsx_ctx* c = dev.ctx();
            BFGSMatB<T> bfgs;
            bfgs.reset(c, m);
            for (int k = 0; k < npairs; k++)
            {
                double sy = 0, yy = 0;
                detail::check(lbfgsx_bfgs_stage_correction_host(c, static_cast<const T*>(S) + size_t(k) * size_t(n),
                                                                static_cast<const T*>(Y) + size_t(k) * size_t(n), &sy, &yy));
                bfgs.add_correction(T(sy), T(yy));
            }
            dev.upload(LBFGSX_VEC_X, static_cast<const T*>(x0));
            dev.upload(LBFGSX_VEC_G, static_cast<const T*>(g));
            dev.upload(LBFGSX_VEC_LB, static_cast<const T*>(lb));
            dev.upload(LBFGSX_VEC_UB, static_cast<const T*>(ub));
            typename Cauchy<T>::Result gcp;
            Cauchy<T>::get_cauchy_point(bfgs, gcp);
            dev.download(LBFGSX_VEC_XCP, static_cast<T*>(xcp));
            for (size_t j = 0; j < gcp.vecc.size(); j++)
                vecc[j] = double(gcp.vecc[j]);
            counts[0] = gcp.nact;
            counts[1] = gcp.nfree;
            counts[2] = gcp.crossings;
            if (state)
                detail::check(lbfgsx_b_download_state(c, state));
            if (drt)
            {
                typename SubspaceMin<T>::Stats st;
                SubspaceMin<T>::subspace_minimize(bfgs, gcp, max_submin, &st);
                counts[3] = st.sweeps;
                dev.download(LBFGSX_VEC_D, static_cast<T*>(drt));
            }
        };
        if (dtype == LBFGSX_F64)
            body(double());
        else
            body(float());
    });
    if (errbuf && errlen > 0)
        std::snprintf(errbuf, size_t(errlen), "%s", r.msg);
    return rc;
}

int lbfgsx_batch_minimize(int algo, int dtype, int linesearch, const lbfgsx_params* p, int objective, int64_t n,
                          int64_t first, int64_t count, uint64_t seed_base, int device, int nthreads,
                          lbfgsx_batch_item* out)
{
    if (count <= 0)
        return LBFGSX_OK;
    if (nthreads < 1)
        nthreads = 1;
    if (nthreads > count)
        nthreads = int(count);
    std::atomic<int64_t> next(0);
    std::atomic<int> fatal(0);
    auto worker = [&]() {
        lbfgsx_solver* s = nullptr;
        if (lbfgsx_solver_create(&s, algo, dtype, linesearch, p, device) != 0 || lbfgsx_solver_prepare(s, n) != 0)
        {
            fatal.store(LBFGSX_E_RUNTIME);
            if (s)
                lbfgsx_solver_destroy(s);
            return;
        }
        lbfgsx_ctx* c = lbfgsx_solver_ctx(s);
        for (;;)
        {
            const int64_t k = next.fetch_add(1);
            if (k >= count)
                break;
            const uint64_t seed = seed_base + uint64_t(first + k);
            int rc = 0;
            if (objective == LBFGSX_OBJ_EXT_ROSENBROCK)
                rc = lbfgsx_gen_rosen_x0(c, seed);
            else
            {
                rc = lbfgsx_gen_diag_quad(c, 10.0, seed);
                if (!rc)
                    rc = lbfgsx_fill(c, LBFGSX_VEC_X, 0.0);
            }
            if (!rc && algo == LBFGSX_ALGO_LBFGSB)
            {
                rc = lbfgsx_fill(c, LBFGSX_VEC_LB, -1.0);
                if (!rc)
                    rc = lbfgsx_fill(c, LBFGSX_VEC_UB, 1.0);
            }
            lbfgsx_result r;
            std::memset(&r, 0, sizeof(r));
            if (!rc)
                lbfgsx_solver_minimize(s, objective, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &r);
            else
                r.status = rc;
            out[k].niter = r.niter;
            out[k].nfev = r.nfev;
            out[k].status = r.status;
            out[k].fx = r.fx;
            out[k].gnorm = r.gnorm;
        }
        lbfgsx_solver_destroy(s);
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; t++)
        pool.emplace_back(worker);
    for (auto& th : pool)
        th.join();
    return fatal.load();
}

}  // extern "C"
// lock-step batch (include/LBFGSBatched.h): L-BFGS, LineSearchMoreThuente or LineSearchNocedalWright, a built-in objective
template <class T, template <class> class LS>
static void lockstep_body(const lbfgsx_params* p, int objective, double kappa, int64_t n, int64_t first, int count,
                          uint64_t seed_base, const std::vector<int>& devs, lbfgsx_batch_item* out, void* x_out)
{
    LBFGSParam<T> param;
    fill_common<T>(param, p);
    param.linesearch = p->linesearch;
    LBFGSBatchedSolver<T, LS> solver(param);
    std::vector<typename LBFGSBatchedSolver<T, LS>::Item> items;
    BatchObjective obj;
    obj.id = objective;
    obj.kappa = kappa;
    if (devs.size() == 1)
        solver.minimize(obj, n, seed_base, first, count, devs[0], items, static_cast<T*>(x_out));
    else
        solver.minimize(obj, n, seed_base, first, count, devs, items, static_cast<T*>(x_out));
    for (int k = 0; k < count; k++)
    {
        out[k].niter = items[size_t(k)].niter;
        out[k].nfev = items[size_t(k)].nfev;
        out[k].status = items[size_t(k)].status;
        out[k].fx = double(items[size_t(k)].fx);
        out[k].gnorm = double(items[size_t(k)].gnorm);
    }
}

extern "C" {

int lbfgsx_batch_minimize_lockstep_ex(int dtype, int linesearch, int objective, double kappa, const lbfgsx_params* p, int64_t n,
                                      int64_t first, int count, uint64_t seed_base, const int* devices, int ndev,
                                      lbfgsx_batch_item* out, void* x_out, char* errbuf, int errlen)
{
    lbfgsx_result r;
    int rc = guarded(&r, [&]() {
        if (!devices || ndev < 1)
            throw std::invalid_argument("lbfgsx_batch_minimize_lockstep: empty device list");
        if (linesearch != LBFGSX_LS_MORE_THUENTE && linesearch != LBFGSX_LS_NOCEDAL_WRIGHT)
            throw std::invalid_argument("lbfgsx_batch_minimize_lockstep: the lock-step batch runs LineSearchMoreThuente or "
                                        "LineSearchNocedalWright (the policies that exist as state machines)");
        if (objective != LBFGSX_OBJ_EXT_ROSENBROCK && objective != LBFGSX_OBJ_DIAG_QUAD)
            throw std::invalid_argument("lbfgsx_batch_minimize_lockstep: unknown built-in objective");
        const std::vector<int> devs(devices, devices + ndev);
        const bool nw = linesearch == LBFGSX_LS_NOCEDAL_WRIGHT;
        if (dtype == LBFGSX_F64)
        {
            if (nw) lockstep_body<double, LineSearchNocedalWright>(p, objective, kappa, n, first, count, seed_base, devs, out, x_out);
            else lockstep_body<double, LineSearchMoreThuente>(p, objective, kappa, n, first, count, seed_base, devs, out, x_out);
        }
        else
        {
            if (nw) lockstep_body<float, LineSearchNocedalWright>(p, objective, kappa, n, first, count, seed_base, devs, out, x_out);
            else lockstep_body<float, LineSearchMoreThuente>(p, objective, kappa, n, first, count, seed_base, devs, out, x_out);
        }
    });
    if (errbuf && errlen > 0)
        std::snprintf(errbuf, size_t(errlen), "%s", r.msg);
    return rc;
}

}  // extern "C"

// A lock-step batch that outlives one minimisation: the LBFGSBatchedSolver and its resident batch for `count` problems of
// dimension n on one device (lbfgsx_lockstep_create), reused by every lbfgsx_lockstep_minimize.
struct lbfgsx_lockstep
{
    int dtype = LBFGSX_F64, linesearch = LBFGSX_LS_MORE_THUENTE, count = 0, device = 0;
    int64_t n = 0;
    lbfgsx_params prm;
    LBFGSParam<double> pd;
    LBFGSParam<float> pf;
    void* solver = nullptr;  // LBFGSBatchedSolver<T, LS>*
    void (*destroy)(void*) = nullptr;
    void (*timing)(void*, int) = nullptr;
    void (*run)(lbfgsx_lockstep*, int, double, uint64_t, int64_t, lbfgsx_batch_item*, void*, double*) = nullptr;
    void (*run_fn)(lbfgsx_lockstep*, const void*, lbfgsx_batch_objective_fn, void*, lbfgsx_batch_item*, void*, double*) = nullptr;
};

template <class T, template <class> class LS>
static void lockstep_bind(lbfgsx_lockstep* h, LBFGSParam<T>& param, int timing)
{
    typedef LBFGSBatchedSolver<T, LS> S;
    fill_common<T>(param, &h->prm);
    param.linesearch = h->prm.linesearch;
    S* s = new S(param);
    h->solver = s;
    h->destroy = [](void* p) { delete static_cast<S*>(p); };
    h->timing = [](void* p, int on) { static_cast<S*>(p)->set_timing(on != 0); };
    s->set_timing(timing != 0);
    s->prepare(h->n, h->count, h->device);
    static const auto report = [](S* sv, const std::vector<typename S::Item>& items, lbfgsx_batch_item* out, double* st) {
        for (size_t k = 0; k < items.size(); k++)
        {
            out[k].niter = items[k].niter;
            out[k].nfev = items[k].nfev;
            out[k].status = items[k].status;
            out[k].fx = double(items[k].fx);
            out[k].gnorm = double(items[k].gnorm);
        }
        if (st)
        {
            st[0] = double(sv->stats.lockstep_iterations);
            st[1] = sv->stats.fused ? 1.0 : 0.0;
            st[2] = sv->stats.kernel_ms;
            st[3] = double(sv->stats.launches);
            st[4] = double(sv->stats.waits);
            st[5] = double(sv->stats.wait_timeouts);
            st[6] = double(sv->stats.user_calls);
            st[7] = 0.0;
        }
    };
    h->run = [](lbfgsx_lockstep* hh, int objective, double kappa, uint64_t seed_base, int64_t first, lbfgsx_batch_item* out,
                void* x_out, double* st) {
        S* sv = static_cast<S*>(hh->solver);
        std::vector<typename S::Item> items;
        BatchObjective obj;
        obj.id = objective;
        obj.kappa = kappa;
        sv->minimize(obj, hh->n, seed_base, first, hh->count, hh->device, items, static_cast<T*>(x_out));
        report(sv, items, out, st);
    };
    h->run_fn = [](lbfgsx_lockstep* hh, const void* x0, lbfgsx_batch_objective_fn eval, void* user, lbfgsx_batch_item* out,
                   void* x_out, double* st) {
        S* sv = static_cast<S*>(hh->solver);
        std::vector<typename S::Item> items;
        BatchPackedFunctor<T> f;
        f.x0 = x0;
        f.eval = [eval, user](int nact, const std::int64_t* ids, const T* X, T* G, std::int64_t ld, double* fx) {
            return eval(user, nact, ids, X, G, ld, fx);
        };
        sv->minimize(f, hh->n, hh->count, hh->device, items, static_cast<T*>(x_out));
        report(sv, items, out, st);
    };
}

extern "C" {

int lbfgsx_lockstep_create(lbfgsx_lockstep** out, int dtype, int linesearch, const lbfgsx_params* p, int64_t n, int count,
                           int device, int timing, char* errbuf, int errlen)
{
    lbfgsx_result r;
    lbfgsx_lockstep* h = nullptr;
    const int rc = guarded(&r, [&]() {
        if (!out || !p || count <= 0 || n <= 0)
            throw std::invalid_argument("lbfgsx_lockstep_create: invalid argument");
        if (linesearch != LBFGSX_LS_MORE_THUENTE && linesearch != LBFGSX_LS_NOCEDAL_WRIGHT)
            throw std::invalid_argument("lbfgsx_lockstep_create: the lock-step batch runs LineSearchMoreThuente or "
                                        "LineSearchNocedalWright (the policies that exist as state machines)");
        if (dtype != LBFGSX_F64 && dtype != LBFGSX_F32)
            throw std::invalid_argument("lbfgsx_lockstep_create: unknown dtype");
        h = new lbfgsx_lockstep();
        h->dtype = dtype;
        h->linesearch = linesearch;
        h->count = count;
        h->device = device;
        h->n = n;
        h->prm = *p;
        const bool nw = linesearch == LBFGSX_LS_NOCEDAL_WRIGHT;
        if (dtype == LBFGSX_F64)
        {
            if (nw) lockstep_bind<double, LineSearchNocedalWright>(h, h->pd, timing);
            else lockstep_bind<double, LineSearchMoreThuente>(h, h->pd, timing);
        }
        else
        {
            if (nw) lockstep_bind<float, LineSearchNocedalWright>(h, h->pf, timing);
            else lockstep_bind<float, LineSearchMoreThuente>(h, h->pf, timing);
        }
    });
    if (errbuf && errlen > 0)
        std::snprintf(errbuf, size_t(errlen), "%s", r.msg);
    if (rc != LBFGSX_OK)
    {
        if (h)
        {
            if (h->solver && h->destroy)
                h->destroy(h->solver);
            delete h;
        }
        return rc;
    }
    *out = h;
    return LBFGSX_OK;
}

int lbfgsx_lockstep_minimize(lbfgsx_lockstep* h, int objective, double kappa, uint64_t seed_base, int64_t first,
                             lbfgsx_batch_item* out, void* x_out, double stats[8], char* errbuf, int errlen)
{
    lbfgsx_result r;
    const int rc = guarded(&r, [&]() {
        if (!h || !out)
            throw std::invalid_argument("lbfgsx_lockstep_minimize: invalid argument");
        if (objective != LBFGSX_OBJ_EXT_ROSENBROCK && objective != LBFGSX_OBJ_DIAG_QUAD)
            throw std::invalid_argument("lbfgsx_lockstep_minimize: unknown built-in objective");
        h->run(h, objective, kappa, seed_base, first, out, x_out, stats);
    });
    if (errbuf && errlen > 0)
        std::snprintf(errbuf, size_t(errlen), "%s", r.msg);
    return rc;
}

int lbfgsx_lockstep_minimize_fn(lbfgsx_lockstep* h, const void* x0, lbfgsx_batch_objective_fn eval, void* user,
                                lbfgsx_batch_item* out, void* x_out, double stats[8], char* errbuf, int errlen)
{
    lbfgsx_result r;
    int rc = LBFGSX_OK;
    if (lbfgsx_device_count() <= 0)  // (no handle can exist: lbfgsx_lockstep_create allocates on the device)
    {
        rc = LBFGSX_E_NOGPU;
        std::snprintf(r.msg, sizeof(r.msg), "lbfgsx_lockstep_minimize_fn: no HIP device available (this library has no CPU fallback)");
    }
    else
        rc = guarded(&r, [&]() {
            if (!h || !x0 || !eval || !out)
                throw std::invalid_argument("lbfgsx_lockstep_minimize_fn: invalid argument");
            h->run_fn(h, x0, eval, user, out, x_out, stats);
        });
    if (errbuf && errlen > 0)
        std::snprintf(errbuf, size_t(errlen), "%s", r.msg);
    return rc;
}

int lbfgsx_lockstep_set_timing(lbfgsx_lockstep* h, int on)
{
    if (!h || !h->solver)
        return LBFGSX_E_INVALID;
    h->timing(h->solver, on);
    return LBFGSX_OK;
}

void lbfgsx_lockstep_destroy(lbfgsx_lockstep* h)
{
    if (!h)
        return;
    if (h->solver && h->destroy)
        h->destroy(h->solver);
    delete h;
}

int lbfgsx_batch_minimize_lockstep_multi(int dtype, const lbfgsx_params* p, int64_t n, int64_t first, int count,
                                         uint64_t seed_base, const int* devices, int ndev, lbfgsx_batch_item* out,
                                         void* x_out, char* errbuf, int errlen)
{
    return lbfgsx_batch_minimize_lockstep_ex(dtype, LBFGSX_LS_MORE_THUENTE, LBFGSX_OBJ_EXT_ROSENBROCK, 10.0, p, n, first, count,
                                             seed_base, devices, ndev, out, x_out, errbuf, errlen);
}

int lbfgsx_batch_minimize_lockstep(int dtype, const lbfgsx_params* p, int64_t n, int64_t first, int count,
                                   uint64_t seed_base, int device, lbfgsx_batch_item* out, void* x_out, char* errbuf,
                                   int errlen)
{
    return lbfgsx_batch_minimize_lockstep_multi(dtype, p, n, first, count, seed_base, &device, 1, out, x_out, errbuf, errlen);
}

int lbfgsx_solver_hessians(lbfgsx_solver* s, double* B, double* H)
{
    lbfgsx_result r;
    int rc = LBFGSX_OK;
    const int g = guarded(&r, [&]() { rc = s->hessians(B, H); });
    return g ? g : rc;
}

int lbfgsx_solver_stats(lbfgsx_solver* s, long long out[8])
{
    for (int k = 0; k < 8; k++)
        out[k] = s->stats[k];
    return LBFGSX_OK;
}

int lbfgsx_solver_stats2(lbfgsx_solver* s, long long out[8])
{
    for (int k = 0; k < 8; k++)
        out[k] = s->stats2[k];
    return LBFGSX_OK;
}

int lbfgsx_solver_stats3(lbfgsx_solver* s, long long out[8])
{
    for (int k = 0; k < 8; k++)
        out[k] = s->stats3[k];
    return LBFGSX_OK;
}

int lbfgsx_solver_set_recursion(lbfgsx_solver* s, int form) { return s->set_recursion(form); }
int lbfgsx_solver_set_direction_scale(lbfgsx_solver* s, double a) { return s->set_direction_scale(a); }
int lbfgsx_solver_set_allreduce(lbfgsx_solver* s, void (*fn)(double*, int, void*), void* user)
{
    return s->set_allreduce(fn, user);
}

int lbfgsx_solver_set_devices(lbfgsx_solver* s, const int* devices, int ndev) { return s->set_devices(devices, ndev); }

int lbfgsx_solver_set_iteration_hook(lbfgsx_solver* s, void (*fn)(int, void*), void* user)
{
    s->set_hook(fn, user);
    return LBFGSX_OK;
}

int lbfgsx_solver_minimize(lbfgsx_solver* s, int objective, int64_t n, const void* a, const void* b, void* x,
                           const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    std::memset(out, 0, sizeof(*out));
    return guarded(out, [&]() { s->minimize(objective, n, a, b, x, lb, ub, trace, out); });
}

int lbfgsx_solver_minimize_fn(lbfgsx_solver* s, int64_t n, lbfgsx_objective_fn fn, void* user, void* x, const void* lb,
                              const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    std::memset(out, 0, sizeof(*out));
    if (lbfgsx_device_count() <= 0)
    {
        out->status = LBFGSX_E_NOGPU;
        std::snprintf(out->msg, sizeof(out->msg), "lbfgsx_solver_minimize_fn: no HIP device available (this library has no CPU fallback)");
        return out->status;
    }
    return guarded(out, [&]() {
        if (!s || !fn || n <= 0)
            throw std::invalid_argument("lbfgsx_solver_minimize_fn: invalid argument");
        s->minimize_fn(n, fn, user, x, lb, ub, trace, out);
    });
}

}  // extern "C"

namespace {

typedef lbfgsx_solver::ObjSpec ObjSpec;

// what every entry point for a compiled objective does around its own checks: the result cleared; what is wrong with the
// request itself said first, with or without a device; then the refusal of a host without one; then the run
template <class Checks, class Run>
int objective_entry(const std::string& name, lbfgsx_result* out, Checks&& checks, Run&& run)
{
    std::memset(out, 0, sizeof(*out));
    if (const int bad = guarded(out, checks))
        return bad;
    if (lbfgsx_device_count() <= 0)
    {
        out->status = LBFGSX_E_NOGPU;
        std::snprintf(out->msg, sizeof(out->msg), "%s: no HIP device available (this library has no CPU fallback)", name.c_str());
        return out->status;
    }
    return guarded(out, run);
}

// the entry point of a lattice form: the handle's form and dtype, then the rules of the form's row (form_table.hpp), which
// also give n.  slabs = 0 on two axes, periodic = 0 for a form without a mask
int minimize_lattice(int form, lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols, int periodic,
                     const void* const p[4], int host_mask, const double c[8], void* x, const void* lb, const void* ub,
                     lbfgsx_trace* trace, lbfgsx_result* out)
{
    const lbfgsx::FormRow& row = lbfgsx::kFormRows[form];
    const std::string name = std::string("lbfgsx_solver_minimize") + row.suffix;
    long long n = 0;
    return objective_entry(
        name, out,
        [&]() {
            if (!s || !obj)
                throw std::invalid_argument(name + ": invalid argument");
            if (lbfgsx_objective_form(obj) != form)
                throw std::invalid_argument(name + ": the handle is not a " + row.name + " (lbfgsx_objective_compile" + row.suffix + ")");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument(name + ": the objective was compiled for the other dtype");
            const int D = lbfgsx_objective_D(obj);
            if (const lbfgsx::LatticeRule bad = lbfgsx::lattice_check(form, D, slabs, rows, cols, periodic, &n))
                throw std::invalid_argument(lbfgsx::lattice_refusal(form, bad, D, slabs, rows, cols, periodic));
        },
        [&]() {
            ObjSpec spec;
            spec.form = form, spec.slabs = slabs, spec.rows = rows, spec.cols = cols, spec.periodic = periodic;
            s->minimize_obj(obj, int64_t(n), spec, p, host_mask, c, x, lb, ub, trace, out);
        });
}

}  // namespace

extern "C" {

int lbfgsx_solver_minimize_obj(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, const void* const p[4], int host_mask,
                               const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                               lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_obj", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_obj: invalid argument");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_obj: the objective was compiled for the other dtype");
            const int K = lbfgsx_objective_K(obj), form = lbfgsx_objective_form(obj);
            if (lbfgsx::kFormRows[form].bound_with)
                throw std::invalid_argument(lbfgsx::unshaped_refusal(form, true));
            if (form == LBFGSX_FORM_CHAIN)
            {
                if (n < K)
                    throw std::invalid_argument("chain objective: n = " + std::to_string(n) + " is less than K = " + std::to_string(K) +
                                                ": there is no term");
            }
            else if (n % K != 0)
                throw std::invalid_argument("term objective: n = " + std::to_string(n) + " is not a multiple of K = " + std::to_string(K));
        },
        [&]() { s->minimize_obj(obj, n, ObjSpec(), p, host_mask, c, x, lb, ub, trace, out); });
}

// ---- the six lattice forms: one entry (minimize_lattice), by the form's row of kFormRows
int lbfgsx_solver_minimize_grid(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, const void* const p[4],
                                int host_mask, const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_GRID, s, obj, 0, rows, cols, 0, p, host_mask, c, x, lb, ub, trace, out);
}
int lbfgsx_solver_minimize_volume(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                  const void* const p[4], int host_mask, const double c[8], void* x, const void* lb, const void* ub,
                                  lbfgsx_trace* trace, lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_VOLUME, s, obj, slabs, rows, cols, 0, p, host_mask, c, x, lb, ub, trace, out);
}
int lbfgsx_solver_minimize_grid_periodic(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                         const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                         const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_GRID_PERIODIC, s, obj, 0, rows, cols, periodic, p, host_mask, c, x, lb, ub, trace, out);
}
int lbfgsx_solver_minimize_volume_periodic(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                           int periodic, const void* const p[4], int host_mask, const double c[8], void* x,
                                           const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_VOLUME_PERIODIC, s, obj, slabs, rows, cols, periodic, p, host_mask, c, x, lb, ub, trace, out);
}
int lbfgsx_solver_minimize_grid_field(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                      const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                      const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_GRID_FIELD, s, obj, 0, rows, cols, periodic, p, host_mask, c, x, lb, ub, trace, out);
}
int lbfgsx_solver_minimize_grid_stencil(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                        const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                        const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return minimize_lattice(LBFGSX_FORM_GRID_STENCIL, s, obj, 0, rows, cols, periodic, p, host_mask, c, x, lb, ub, trace, out);
}

int lbfgsx_solver_minimize_graph(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t E, const int32_t* ei,
                                 const int32_t* ej, int edges_on_device, const void* const p[4], int host_mask,
                                 const int64_t counts[4], const double c[8], void* x, const void* lb, const void* ub,
                                 lbfgsx_trace* trace, lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_graph", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_graph: invalid argument");
            if (lbfgsx_objective_form(obj) == LBFGSX_FORM_MESH)
                throw std::invalid_argument("lbfgsx_solver_minimize_graph: the handle is a mesh objective: it is minimised with its "
                                            "elements, lbfgsx_solver_minimize_mesh");
            if (lbfgsx_objective_form(obj) != LBFGSX_FORM_GRAPH)
                throw std::invalid_argument("lbfgsx_solver_minimize_graph: the handle is not a graph objective (lbfgsx_objective_compile_graph)");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_graph: the objective was compiled for the other dtype");
            if (E < 1 || !ei || !ej)
                throw std::invalid_argument("graph objective: E = " + std::to_string(E) +
                                            ": a graph objective has at least one edge (E >= 1) and both index arrays");
        },
        [&]() {
            ObjSpec gr;
            gr.form = LBFGSX_FORM_GRAPH, gr.E = E, gr.ei = ei, gr.ej = ej, gr.on_device = edges_on_device, gr.counts = counts;
            s->minimize_obj(obj, n, gr, p, host_mask, c, x, lb, ub, trace, out);
        });
}

int lbfgsx_solver_minimize_mesh(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t E, const int32_t* elems,
                                int elems_on_device, const void* const p[4], int host_mask, const int64_t counts[4],
                                const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_mesh", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_mesh: invalid argument");
            if (lbfgsx_objective_form(obj) != LBFGSX_FORM_MESH)
                throw std::invalid_argument("lbfgsx_solver_minimize_mesh: the handle is not a mesh objective (lbfgsx_objective_compile_mesh)");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_mesh: the objective was compiled for the other dtype");
            if (E < 1 || !elems)
                throw std::invalid_argument("mesh objective: E = " + std::to_string(E) +
                                            ": a mesh objective has at least one element (E >= 1) and its connectivity table");
            const int D = lbfgsx_objective_dim(obj);
            if (n % D != 0)
                throw std::invalid_argument("mesh objective: n = " + std::to_string(n) + " is not a multiple of D = " + std::to_string(D) +
                                            ": x holds D unknowns per node");
        },
        [&]() {
            ObjSpec gr;
            gr.form = LBFGSX_FORM_MESH, gr.E = E, gr.on_device = elems_on_device, gr.counts = counts, gr.elems = elems;
            s->minimize_obj(obj, n, gr, p, host_mask, c, x, lb, ub, trace, out);
        });
}

int lbfgsx_solver_minimize_linear(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, int64_t nnz,
                                  const int32_t* rowptr, const int32_t* col, const void* val, int matrix_on_device, int lanes,
                                  const void* const p[4], int host_mask, const int64_t counts[4], const double c[8], void* x,
                                  const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_linear", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear: invalid argument");
            const bool multi = lbfgsx_objective_form(obj) == LBFGSX_FORM_LINEAR_MULTI;
            if (lbfgsx_objective_form(obj) != LBFGSX_FORM_LINEAR && !multi)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear: the handle is not a linear-model objective "
                                            "(lbfgsx_objective_compile_linear)");
            if (multi && n % lbfgsx_objective_dim(obj) != 0)
                throw std::invalid_argument("multi-output linear-model objective: n = " + std::to_string(n) +
                                            " is not a multiple of D = " + std::to_string(lbfgsx_objective_dim(obj)) +
                                            ": x holds the D weights of each feature");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear: the objective was compiled for the other dtype");
            if (R < 1 || nnz < 1 || !rowptr || !col || !val)
                throw std::invalid_argument("linear-model objective: R = " + std::to_string(R) + ", nnz = " + std::to_string(nnz) +
                                            ": a linear-model objective has at least one row and one entry (R >= 1, nnz >= 1) and "
                                            "its three CSR arrays");
        },
        [&]() {
            ObjSpec gr;
            gr.form = LBFGSX_FORM_LINEAR, gr.on_device = matrix_on_device, gr.counts = counts;
            gr.R = R, gr.nnz = nnz, gr.rowptr = rowptr, gr.col = col, gr.val = val, gr.lanes = lanes;
            s->minimize_obj(obj, n, gr, p, host_mask, c, x, lb, ub, trace, out);
        });
}

int lbfgsx_solver_minimize_linear_graph(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, int64_t nnz,
                                        const int32_t* rowptr, const int32_t* col, const void* val, int matrix_on_device,
                                        int lanes, int64_t E, const int32_t* ei, const int32_t* ej, int edges_on_device,
                                        const void* const p[4], int host_mask, const int64_t counts[4], const double c[8],
                                        void* x, const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_linear_graph", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear_graph: invalid argument");
            if (lbfgsx_objective_form(obj) != LBFGSX_FORM_LINEAR_GRAPH)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear_graph: the handle is not a graph-regularised linear-model "
                                            "objective (lbfgsx_objective_compile_linear_graph)");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_linear_graph: the objective was compiled for the other dtype");
            if (E < 1 || !ei || !ej)
                throw std::invalid_argument("graph-regularised linear-model objective: E = " + std::to_string(E) +
                                            ": a graph-regularised linear-model objective has at least one edge (E >= 1) and both "
                                            "index arrays");
            if (R < 1 || nnz < 1 || !rowptr || !col || !val)
                throw std::invalid_argument("graph-regularised linear-model objective: R = " + std::to_string(R) + ", nnz = " +
                                            std::to_string(nnz) + ": a linear-model objective has at least one row and one entry "
                                            "(R >= 1, nnz >= 1) and its three CSR arrays");
        },
        [&]() {
            ObjSpec gr;
            gr.form = LBFGSX_FORM_LINEAR_GRAPH, gr.E = E, gr.ei = ei, gr.ej = ej, gr.on_device = matrix_on_device, gr.counts = counts;
            gr.R = R, gr.nnz = nnz, gr.rowptr = rowptr, gr.col = col, gr.val = val, gr.lanes = lanes, gr.edges_dev = edges_on_device;
            s->minimize_obj(obj, n, gr, p, host_mask, c, x, lb, ub, trace, out);
        });
}

int lbfgsx_solver_minimize_dense(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, const void* A, int64_t lda,
                                 int a_on_device, int lanes, const void* const p[4], int host_mask, const int64_t counts[4],
                                 const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                 lbfgsx_result* out)
{
    return objective_entry(
        "lbfgsx_solver_minimize_dense", out,
        [&]() {
            if (!s || !obj || n <= 0)
                throw std::invalid_argument("lbfgsx_solver_minimize_dense: invalid argument");
            if (lbfgsx_objective_form(obj) != LBFGSX_FORM_DENSE)
                throw std::invalid_argument("lbfgsx_solver_minimize_dense: the handle is not a dense linear-model objective "
                                            "(lbfgsx_objective_compile_dense)");
            const int D = lbfgsx_objective_dim(obj);
            if (n % D != 0)
                throw std::invalid_argument("dense linear-model objective: n = " + std::to_string(n) + " is not a multiple of D = " +
                                            std::to_string(D) + ": x holds the D weights of each feature");
            if (lbfgsx_objective_dtype(obj) != s->dtype)
                throw std::invalid_argument("lbfgsx_solver_minimize_dense: the objective was compiled for the other dtype");
            if (R < 1)
                throw std::invalid_argument("dense linear-model objective: R = " + std::to_string(R) +
                                            ": a dense linear-model objective has at least one row (R >= 1)");
            if (!A)
                throw std::invalid_argument("dense linear-model objective: A is null: a dense linear-model objective has its R x F "
                                            "matrix (R = " + std::to_string(R) + ")");
            if (lda < n / D)
                throw std::invalid_argument("dense linear-model objective: lda = " + std::to_string(lda) + " is less than F = n / D = " +
                                            std::to_string(n / D) + ": a row of the matrix holds its F values first");
        },
        [&]() {
            ObjSpec gr;
            gr.form = LBFGSX_FORM_DENSE, gr.on_device = a_on_device, gr.counts = counts;
            gr.R = R, gr.A = A, gr.lda = lda, gr.lanes = lanes;
            s->minimize_obj(obj, n, gr, p, host_mask, c, x, lb, ub, trace, out);
        });
}
}
