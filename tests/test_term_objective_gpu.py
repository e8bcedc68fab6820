"""GPU suite: term objectives compiled at run time and evaluated inside the fused kernels (lbfgspp_amd.TermObjective,
lbfgsx_solver_minimize_obj).  A re-statement of a built-in objective runs the same kernel text with the same flags and the
same sums, so it is compared with the built-in bit for bit; the comparisons with the oracle use the assertions of the built-in
trajectory tests (tests/test_lbfgs_gpu.py, tests/test_lbfgsb_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_term_objective_cpu import QUAD, ROSEN

pytestmark = pytest.mark.gpu
TOL = {O.F64: 1e-10, O.F32: 1e-4}  # tests/test_lbfgs_gpu.py (BASELINE.json north_star tolerances, iterate parity)

# f(x) = sum_i p0_i (x_i - p1_i)^2 + c0 (x_i - p1_i)^4: separable, strongly convex, minimiser p1
QUARTIC = """const T d = x[0] - p1[i];
const T d2 = d * d;
g[0] = T(2) * p0[i] * d + T(4) * c[0] * (d2 * d);
return p0[i] * d2 + c[0] * (d2 * d2);"""


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1
    return A


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _counters(core, reset=0):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), reset) == 0
    return list(cnt)


def _solve(A, solver, f, x0, bounds=(), cap=600):
    """one minimise with a trace; an exception of the solver is part of the outcome (both forms must raise the same)"""
    n = x0.size
    stride = max(1, n // 4096)
    tr = A.TraceBuffer(n, cap=cap, stride=stride)
    x = x0.copy()
    err = None
    try:
        solver.minimize(f, x, *bounds, trace=tr)
    except (ValueError, ArithmeticError, RuntimeError) as e:
        err = (type(e).__name__, str(e))
    r = solver.last
    return dict(x=x, niter=r.niter, nfev=r.nfev, fx=r.fx, gnorm=r.gnorm, err=err, count=tr.count, fxs=tr.fx[:tr.count].copy(),
                xs=tr.xs[:tr.count].copy())


def _assert_same_bits(a, b):
    assert a["err"] == b["err"]
    assert (a["niter"], a["nfev"], a["count"]) == (b["niter"], b["nfev"], b["count"])
    assert a["fx"] == b["fx"] or (np.isnan(a["fx"]) and np.isnan(b["fx"]))
    assert a["gnorm"] == b["gnorm"] or (np.isnan(a["gnorm"]) and np.isnan(b["gnorm"]))
    assert np.array_equal(a["x"], b["x"], equal_nan=True)
    assert np.array_equal(a["fxs"], b["fxs"], equal_nan=True)
    assert np.array_equal(a["xs"], b["xs"], equal_nan=True)


LINESEARCHES = [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR]


@pytest.mark.parametrize("m", [1, 6, 140])
@pytest.mark.parametrize("n", [2, 4096 + 2, 1_000_002])
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("ls", LINESEARCHES)
def test_rosenbrock_restated_is_bit_identical_to_the_builtin(A, ls, dtype, n, m):
    dt = O.NPDT[dtype]
    x0 = O.rosen_x0(n, 7, dtype)
    p = dict(m=m, max_iterations=25)
    builtin = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt), A.ExtendedRosenbrock(), x0)
    term = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt), A.TermObjective(ROSEN, K=2), x0)
    assert builtin["nfev"] >= 1 and builtin["count"] == builtin["nfev"]
    _assert_same_bits(builtin, term)


@pytest.mark.parametrize("m", [1, 6, 140])
@pytest.mark.parametrize("n", [2, 4096 + 2, 1_000_002])
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("ls", LINESEARCHES)
def test_quadratic_restated_is_bit_identical_to_the_builtin(A, ls, dtype, n, m):
    dt = O.NPDT[dtype]
    a, b = O.quad_problem(n, 10.0, 1, dtype)
    x0 = np.zeros(n, dt)
    p = dict(m=m, max_iterations=25)
    builtin = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt), A.DiagQuadratic(a, b), x0)
    term = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt), A.TermObjective(QUAD, data=(a, b)), x0)
    assert builtin["count"] == builtin["nfev"] >= 1
    _assert_same_bits(builtin, term)


@pytest.mark.parametrize("m", [3, 10])
@pytest.mark.parametrize("n,iters", [(2000, 15), (20000, 25)])
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
def test_box_quadratic_restated_is_bit_identical_to_the_builtin(A, dtype, n, iters, m):
    """the box instances of tests/test_lbfgsb_gpu.py (_traj), statistics of the solver included"""
    dt = O.NPDT[dtype]
    a, b = O.quad_problem(n, 10.0, 1, dtype)
    lb, ub = -np.ones(n, dt), np.ones(n, dt)
    prm = dict(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters)
    s1 = A.LBFGSBSolver(A.LBFGSBParam(**prm), dtype=dt)
    builtin = _solve(A, s1, A.DiagQuadratic(a, b), np.zeros(n, dt), (lb, ub))
    s2 = A.LBFGSBSolver(A.LBFGSBParam(**prm), dtype=dt)
    term = _solve(A, s2, A.TermObjective(QUAD, data=(a, b)), np.zeros(n, dt), (lb, ub))
    _assert_same_bits(builtin, term)
    st1, st2 = s1.stats(), s2.stats()
    for key in ("gcp_crossings", "submin_sweeps", "submin_calls", "submin_unconverged", "resets", "gcp_searches"):
        assert st1[key] == st2[key], key
    assert st1["submin_sweeps"] > 0


@pytest.mark.parametrize("m", [3, 10])
def test_box_rosenbrock_restated_is_bit_identical_to_the_builtin(A, m):
    n = 20000
    x0 = O.rosen_x0(n)
    lb, ub = -0.5 * np.ones(n), 0.9 * np.ones(n)
    prm = dict(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=30)
    s1, s2 = A.LBFGSBSolver(A.LBFGSBParam(**prm)), A.LBFGSBSolver(A.LBFGSBParam(**prm))
    builtin = _solve(A, s1, A.ExtendedRosenbrock(), x0, (lb, ub))
    term = _solve(A, s2, A.TermObjective(ROSEN, K=2), x0, (lb, ub))
    _assert_same_bits(builtin, term)
    st1, st2 = s1.stats(), s2.stats()
    assert (st1["gcp_crossings"], st1["submin_sweeps"]) == (st2["gcp_crossings"], st2["submin_sweeps"])


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT])
def test_rosenbrock_term_follows_the_oracle_f64(A, oracle, ls):
    """as test_trajectory_rosenbrock_f64 (its first case), through tests/test_user_objective_gpu.py's form of it"""
    n, m, iters = 20000, 10, 60
    x0 = O.rosen_x0(n)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgs(O.F64, ls, O.OBJ_ROSEN, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters),
                                trace=tr_ref)
    s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), linesearch=ls)
    tr = A.TraceBuffer(n, cap=1024)
    x = x0.copy()
    niter, fx = s.minimize(A.TermObjective(ROSEN, K=2), x, trace=tr)
    assert r_ref.status == 0 and (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert tr.count == k
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= TOL[O.F64]
    assert np.abs(x - x_ref).max() <= TOL[O.F64]


def test_box_quadratic_term_follows_the_oracle(A, oracle, tol=1e-10):
    """as test_trajectory_box_quadratic_f64 (tests/test_lbfgsb_gpu.py), its first instance"""
    if not oracle.supports_lbfgsb:
        pytest.skip("this oracle build has no L-BFGS-B entry points")
    n, m, iters = 2000, 6, 15
    a, b = O.quad_problem(n, 10.0, 1)
    lb, ub = -np.ones(n), np.ones(n)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgsb(O.F64, O.OBJ_QUAD, np.zeros(n), lb, ub,
                                 O.lbfgsb_params(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters), a=a, b=b, trace=tr_ref)
    s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
    tr = A.TraceBuffer(n, cap=1024)
    x = np.zeros(n)
    niter, fx = s.minimize(A.TermObjective(QUAD, data=(a, b)), x, lb, ub, trace=tr)
    assert (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert tr.count == k
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= tol
    assert np.abs(x - x_ref).max() <= tol
    assert np.array_equal(np.abs(x) == 1.0, np.abs(x_ref) == 1.0)
    assert abs(fx - r_ref.fx) <= 1e-12 * abs(r_ref.fx)


def _quartic_instance(n=100_000):
    rng = np.random.default_rng(20260)
    return 1.0 + 9.0 * rng.random(n), 2.0 * rng.random(n) - 1.0, 0.5


def _quartic_torch(torch, p0, p1, c0):
    t0, t1 = torch.as_tensor(p0, device="cuda:0"), torch.as_tensor(p1, device="cuda:0")

    def fn(x, g):
        d = x - t1
        d2 = d * d
        torch.add(2.0 * t0 * d, d2 * d, alpha=4.0 * c0, out=g)
        return float((t0 * d2 + c0 * d2 * d2).sum())
    return fn


@pytest.mark.parametrize("form", ["term", "torch"])
def test_unseen_objective_lbfgs_reaches_its_minimiser(A, torch, form):
    """f = sum p0 (x - p1)^2 + c0 (x - p1)^4, p0 in [1, 10]: |x_i - p1_i| <= |g_i| / (2 p0_i) <= |g_i| / 2 per coordinate, hence
    ||x - p1||_2 <= ||g||_2 / 2 <= epsilon / 2 once the run has ended by the gradient test.  epsilon = 1e-8 as the issue sets it."""
    eps = 1e-8
    p0, p1, c0 = _quartic_instance()
    n = p0.size
    f = A.TermObjective(QUARTIC, data=(p0, p1), scalars=(c0,)) if form == "term" else A.DeviceObjective(_quartic_torch(torch, p0, p1, c0))
    s = A.LBFGSSolver(A.LBFGSParam(epsilon=eps, epsilon_rel=0, past=0))
    x = np.zeros(n)
    niter, fx = s.minimize(f, x)
    dist = float(np.linalg.norm(x - p1))
    print("%s: niter %d nfev %d fx %.3g |g| %.3g ||x - p1|| %.3g" % (form, niter, s.last.nfev, fx, s.final_grad_norm(), dist))
    assert s.final_grad_norm() <= eps
    assert dist <= eps / 2


def test_unseen_objective_lbfgsb_reaches_its_minimiser(A):
    """the same objective with lb = p1 + 0.1 on every third coordinate: the stopping quantity is the max-norm of the projected
    gradient, so per coordinate: the bounded ones sit on their bound, every free one within |g_i| / 2 <= epsilon / 2 of p1_i.
    epsilon = 1e-6, past = 0 as the issue sets them."""
    eps = 1e-6
    p0, p1, c0 = _quartic_instance()
    n = p0.size
    lb = np.full(n, -np.inf)
    lb[::3] = p1[::3] + 0.1
    ub = np.full(n, np.inf)
    s = A.LBFGSBSolver(A.LBFGSBParam(epsilon=eps, epsilon_rel=0, past=0))
    x = np.zeros(n)
    niter, fx = s.minimize(A.TermObjective(QUARTIC, data=(p0, p1), scalars=(c0,)), x, lb, ub)
    free = np.ones(n, bool)
    free[::3] = False
    print("niter %d nfev %d fx %.6g projected |g|_inf %.3g max free |x - p1| %.3g" % (niter, s.last.nfev, fx, s.final_grad_norm(),
                                                                                   np.abs(x - p1)[free].max()))
    assert s.final_grad_norm() <= eps
    assert np.array_equal(x[::3], lb[::3])
    assert np.abs(x - p1)[free].max() <= eps / 2


def test_term_objective_takes_the_fused_launches(A, torch):
    """launch counters of the library (lbfgsx_counters_ex) over one whole minimise: a term objective costs what the built-in
    costs -- the trial is ONE launch that forms the point, evaluates and reduces (the single-problem L-BFGS path has no
    speculative first trial inside the persistent launch, so there is no launch to except) -- and less than the callable,
    which needs the trial point and grad . drt around every call."""
    core, _ = A.load()
    n, m, iters = 200_000, 6, 20
    x0 = O.rosen_x0(n)
    prm = dict(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters)

    def rosen(x, g):
        x0_, x1_ = x[0::2], x[1::2]
        t1 = 1.0 - x0_
        t2 = 10.0 * (x1_ - x0_ * x0_)
        g1 = 20.0 * t2
        g[1::2] = g1
        g[0::2] = -2.0 * (x0_ * g1 + t1)
        return float((t1 * t1 + t2 * t2).sum(dtype=torch.float64))

    launches, runs = {}, {}
    for name, f in (("builtin", A.ExtendedRosenbrock()), ("term", A.TermObjective(ROSEN, K=2)), ("torch", A.DeviceObjective(rosen))):
        s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x)
        c1 = _counters(core)
        launches[name] = c1[0] - c0[0]
        runs[name] = (niter, s.last.nfev)
    print(launches, runs)
    assert runs["builtin"] == runs["term"] == runs["torch"]
    assert launches["term"] == launches["builtin"]
    # two launches of the library per evaluation in place of one (the initial evaluation: one in place of one)
    assert launches["torch"] >= launches["term"] + runs["term"][1] - 1


def test_lbfgsb_term_objective_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    n, m, iters = 20000, 6, 25
    a, b = O.quad_problem(n, 10.0, 1)
    lb, ub = -np.ones(n), np.ones(n)
    out = {}
    for name, f in (("builtin", A.DiagQuadratic(a, b)), ("term", A.TermObjective(QUAD, data=(a, b)))):
        s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
        s.prepare(n)
        x = np.zeros(n)
        c0 = _counters(core)
        s.minimize(f, x, lb, ub)
        c1 = _counters(core)
        ahead = (C.c_int64 * 2)()
        assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
        out[name] = (c1[0] - c0[0], ahead[0], ahead[1])
    print(out)
    assert out["term"][1] > 0 and out["term"][2] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["term"] == out["builtin"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_data_is_used_in_place_and_rebinding_does_not_recompile(A, torch, dtype):
    n = 50_000
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(3)
    p0 = (1.0 + rng.random(n)).astype(dtype)
    p1 = (rng.random(n) - 0.5).astype(dtype)
    f = A.TermObjective(QUARTIC, data=(torch.as_tensor(p0, device="cuda:0"), torch.as_tensor(p1, device="cuda:0")), scalars=(0.5,))
    s = A.LBFGSSolver(A.LBFGSParam(epsilon=1e-4, epsilon_rel=0), dtype=dtype)
    x = torch.zeros(n, dtype=tdt, device="cuda:0")
    s.minimize(f, x)
    bound = s.bound_data()
    assert bound[:2] == [f.data[0].data_ptr(), f.data[1].data_ptr()] and bound[2:] == [0, 0]
    tol = 1e-4 if dtype == np.float64 else 1e-3
    assert np.abs(x.cpu().numpy() - p1).max() <= tol
    handle = f._h[0 if dtype == np.float64 else 1].value
    # numpy data: uploaded into buffers of the context, not read in place
    q1 = (p1 + 0.25).astype(dtype)
    f.set_data(p0, q1)
    xn = np.zeros(n, dtype)
    s.minimize(f, xn)
    bound2 = s.bound_data()
    assert bound2[0] not in (0, p0.ctypes.data) and bound2[1] not in (0, q1.ctypes.data) and bound2[:2] != bound[:2]
    assert np.abs(xn - q1).max() <= tol
    # other device arrays on the same solver: bound in place again, the compiled code kept
    t1 = torch.as_tensor((p1 - 0.25).astype(dtype), device="cuda:0")
    f.set_data(f_p0 := torch.as_tensor(p0, device="cuda:0"), t1)
    x.zero_()
    s.minimize(f, x)
    assert s.bound_data()[:2] == [f_p0.data_ptr(), t1.data_ptr()]
    assert np.abs(x.cpu().numpy() - (p1 - 0.25).astype(dtype)).max() <= tol
    assert f._h[0 if dtype == np.float64 else 1].value == handle
    assert A.TermObjective(QUARTIC).info(dtype)["cache_hit"]


def test_data_of_another_dtype_or_layout_is_converted_and_kept_alive(A):
    """numpy data that is not already a contiguous array of the solver's dtype (float64 arrays and a list for an f32 solver, a
    strided view) is converted on the way in; the converted copies -- several of them, each large enough to be returned to the
    system when freed -- must live until the library has read them.  Same result as with ready-made float32 arrays, bit for bit."""
    n = 1_000_002
    rng = np.random.default_rng(11)
    p0 = 1.0 + rng.random(n)
    wide = np.empty((n, 2))
    wide[:, 0] = rng.random(n) - 0.5
    p1_view = wide[:, 0]  # float64, strided
    assert p0.dtype == np.float64 and not p1_view.flags["C_CONTIGUOUS"]
    prm = dict(m=6, epsilon=0, epsilon_rel=0, max_iterations=12)
    runs = []
    for data in ((p0, p1_view), (p0.astype(np.float32), np.ascontiguousarray(p1_view, np.float32)), (p0.tolist(), p1_view)):
        s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE, dtype=np.float32)
        runs.append(_solve(A, s, A.TermObjective(QUARTIC, data=data, scalars=(0.5,)), np.zeros(n, np.float32)))
    assert runs[0]["niter"] == 12 and runs[0]["err"] is None
    _assert_same_bits(runs[1], runs[0])
    _assert_same_bits(runs[1], runs[2])
    assert np.abs(runs[0]["x"] - p1_view).max() <= 1e-3
    # L-BFGS-B takes the same route
    lb, ub = np.full(n, -0.25, np.float32), np.full(n, 0.25, np.float32)
    prb = dict(m=6, epsilon=0, epsilon_rel=0, past=0, max_iterations=8)
    rb = []
    for data in ((p0, p1_view), (p0.astype(np.float32), np.ascontiguousarray(p1_view, np.float32))):
        s = A.LBFGSBSolver(A.LBFGSBParam(**prb), dtype=np.float32)
        rb.append(_solve(A, s, A.TermObjective(QUARTIC, data=data, scalars=(0.5,)), np.zeros(n, np.float32), (lb, ub)))
    _assert_same_bits(rb[1], rb[0])


def test_a_slot_left_empty_is_not_bound_to_an_earlier_upload(A):
    n = 4096
    s = A.LBFGSSolver(A.LBFGSParam(epsilon=1e-6, epsilon_rel=0))
    p0, p1 = np.full(n, 2.0), np.linspace(-1, 1, n)
    s.minimize(A.TermObjective(QUARTIC, data=(p0, p1), scalars=(0.5,)), np.zeros(n))
    assert all(s.bound_data()[:2]) and s.bound_data()[2:] == [0, 0]
    s.minimize(A.TermObjective(ROSEN, K=2), O.rosen_x0(n))
    assert s.bound_data() == [0, 0, 0, 0]


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(A.TermObjective(ROSEN, K=2), O.rosen_x0(1000))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(A.TermObjective(ROSEN, K=2), O.rosen_x0(1000))
