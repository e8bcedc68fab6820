"""GPU suite: a caller-supplied objective on device memory for the single-problem solvers (lbfgsx_solver_minimize_fn,
lbfgspp_amd.DeviceObjective).  The callables below are plain torch code (separate element-wise ops); f is summed by the caller,
not by the library, so the comparisons with the oracle use the tolerances of the built-in trajectory tests
(tests/test_lbfgs_gpu.py, tests/test_lbfgsb_gpu.py), not bit-identity."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
TOL = {O.F64: 1e-10, O.F32: 1e-4}  # tests/test_lbfgs_gpu.py (BASELINE.json north_star tolerances, iterate parity)


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


def quad_fn(torch, a, b, dtype=np.float64):
    """f = 0.5 |a.*x - b|^2, grad = a.*(a.*x - b), element by element as the oracle's quadratic.  Near the minimiser an ulp of
    x moves f by ~1e-13 of its value (the residuals cancel), and the built-in trajectory test holds every f to 1e-13 of the
    oracle's: a callable held to that bound has to round its sum as the oracle does, so the terms are summed exactly
    (math.fsum) rather than by torch's tree reduction."""
    import math
    at, bt = torch.as_tensor(a.astype(dtype), device="cuda:0"), torch.as_tensor(b.astype(dtype), device="cuda:0")

    def fn(x, g):
        r = at * x - bt
        torch.mul(at, r, out=g)
        return 0.5 * math.fsum((r * r).double().cpu().tolist())
    return fn


def rosen_fn(torch):
    """the reference's examples/example-rosenbrock.cpp, pair by pair"""
    def fn(x, g):
        x0, x1 = x[0::2], x[1::2]
        t1 = 1.0 - x0
        t2 = 10.0 * (x1 - x0 * x0)
        g1 = 20.0 * t2
        g[1::2] = g1
        g[0::2] = -2.0 * (x0 * g1 + t1)
        return float((t1 * t1 + t2 * t2).sum(dtype=torch.float64))
    return fn


def _run(A, dtype, ls, fn, x0, m, iters, cap=1024, **pk):
    n = x0.size
    s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters, **pk), linesearch=ls, dtype=O.NPDT[dtype])
    tr = A.TraceBuffer(n, cap=cap)
    x = np.array(x0, dtype=O.NPDT[dtype])
    niter, fx = s.minimize(A.DeviceObjective(fn), x, trace=tr)
    return s, x, niter, fx, tr


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR])
def test_torch_quadratic_follows_the_oracle_f64(A, torch, oracle, ls):
    """as test_trajectory_quadratic_f64"""
    n = 20000
    a, b = O.quad_problem(n)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgs(O.F64, ls, O.OBJ_QUAD, np.zeros(n), O.lbfgs_params(m=10, epsilon=0, epsilon_rel=0, max_iterations=40),
                                a=a, b=b, trace=tr_ref)
    s, x, niter, fx, tr = _run(A, O.F64, ls, quad_fn(torch, a, b), np.zeros(n), 10, 40)
    assert r_ref.status == 0 and (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert tr.count == k
    print("ls %d: max |dx| over the trace %.3g, final %.3g, max relative |df| %.3g"
          % (ls, np.abs(tr.xs[:k] - tr_ref.xs[:k]).max(), np.abs(x - x_ref).max(),
             (np.abs(tr.fx[:k] - tr_ref.fx[:k]) / np.abs(tr_ref.fx[:k])).max()))
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= TOL[O.F64]
    assert np.abs(x - x_ref).max() <= TOL[O.F64]
    assert np.allclose(tr.fx[:k], tr_ref.fx[:k], rtol=1e-13, atol=0)


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT])
def test_torch_rosenbrock_follows_the_oracle_f64(A, torch, oracle, ls):
    """as test_trajectory_rosenbrock_f64 (its first case)"""
    n, m, iters = 20000, 10, 60
    x0 = O.rosen_x0(n)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgs(O.F64, ls, O.OBJ_ROSEN, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters),
                                trace=tr_ref)
    s, x, niter, fx, tr = _run(A, O.F64, ls, rosen_fn(torch), x0, m, iters)
    assert r_ref.status == 0 and (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= TOL[O.F64]
    assert np.abs(x - x_ref).max() <= TOL[O.F64]


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR])
def test_torch_rosenbrock_follows_the_oracle_f32(A, torch, oracle, ls):
    """as test_trajectory_rosenbrock_f32, for every line search"""
    n = 100000
    x0 = O.rosen_x0(n, 1000, O.F32)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgs(O.F32, ls, O.OBJ_ROSEN, x0, O.lbfgs_params(m=10, epsilon=0, epsilon_rel=0, max_iterations=30),
                                trace=tr_ref)
    s, x, niter, fx, tr = _run(A, O.F32, ls, rosen_fn(torch), x0, 10, 30)
    assert (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= TOL[O.F32]
    assert np.abs(x.astype(np.float64) - x_ref.astype(np.float64)).max() <= TOL[O.F32]


@pytest.mark.parametrize("n,m,iters", [(2000, 6, 15), (20000, 10, 25)])
def test_torch_box_quadratic_follows_the_oracle(A, torch, oracle, n, m, iters, tol=1e-10):
    """as test_trajectory_box_quadratic_f64 (tests/test_lbfgsb_gpu.py)"""
    if not oracle.supports_lbfgsb:
        pytest.skip("this oracle build has no L-BFGS-B entry points")
    a, b = O.quad_problem(n, 10.0, 1)
    lb, ub = -np.ones(n), np.ones(n)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgsb(O.F64, O.OBJ_QUAD, np.zeros(n), lb, ub,
                                 O.lbfgsb_params(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters), a=a, b=b, trace=tr_ref)
    s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
    tr = A.TraceBuffer(n, cap=1024)
    x = np.zeros(n)
    niter, fx = s.minimize(A.DeviceObjective(quad_fn(torch, a, b)), x, lb, ub, trace=tr)
    assert (niter, s.last.nfev) == (r_ref.niter, r_ref.nfev)
    k = tr_ref.count
    assert tr.count == k
    assert np.abs(tr.xs[:k] - tr_ref.xs[:k]).max() <= tol
    assert np.abs(x - x_ref).max() <= tol
    assert np.array_equal(np.abs(x) == 1.0, np.abs(x_ref) == 1.0)
    assert abs(fx - r_ref.fx) <= 1e-12 * abs(r_ref.fx)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_callback_tensors_alias_the_context_vectors_and_the_library_adds_no_launch(A, torch, dtype):
    """zero copy: x / grad inside the callback ARE LBFGSX_VEC_X / _G at the first evaluation and LBFGSX_VEC_XT / _GT at every
    trial, on the solver's device.  And the library's own statements around a callback are the device-functor path's
    (LBFGSpp/Device.h, Evaluator::trial): between two trials of one line search it launches the trial point and grad . drt,
    i.e. two kernels (lbfgsx_counters_ex) -- nothing more for having gone through the C ABI."""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    n = 5000
    s = A.LBFGSSolver(A.LBFGSParam(m=5, epsilon=0, epsilon_rel=0, max_iterations=12), linesearch=A.LS_MORE_THUENTE, dtype=dtype)
    inner = rosen_fn(torch)
    seen = []

    def fn(x, g):
        cnt = (C.c_int64 * 8)()
        core.lbfgsx_counters_ex(C.byref(cnt), 0)
        vec = [core.lbfgsx_vec(s.ctx, w) for w in (L.VEC_X, L.VEC_G, L.VEC_XT, L.VEC_GT)]
        seen.append((x.data_ptr(), g.data_ptr(), vec, cnt[0], str(x.device), x.dtype, x.shape[0]))
        return inner(x, g)

    x = O.rosen_x0(n).astype(dtype)
    niter, fx = s.minimize(A.DeviceObjective(fn), x)
    assert len(seen) == s.last.nfev > niter  # some search took more than one trial
    want = torch.float64 if dtype == np.float64 else torch.float32
    for k, (xp, gp, vec, _, dev, dt, nn) in enumerate(seen):
        assert (xp, gp) == ((vec[0], vec[1]) if k == 0 else (vec[2], vec[3])), k
        assert dev == "cuda:0" and dt == want and nn == n
    gaps = np.diff([c[3] for c in seen])
    assert gaps.min() == 2, gaps


def test_exception_in_the_callback_reaches_the_caller_and_the_solver_goes_on(A, torch):
    from lbfgspp_amd import _lib as L
    n, kth = 1000, 4
    inner = rosen_fn(torch)
    calls = [0]

    def fn(x, g):
        calls[0] += 1
        if calls[0] == kth:
            raise KeyError("call %d" % kth)
        return inner(x, g)

    for make in (lambda: A.LBFGSSolver(A.LBFGSParam(max_iterations=30), linesearch=A.LS_MORE_THUENTE),
                 lambda: A.LBFGSBSolver(A.LBFGSBParam(max_iterations=30))):
        s = make()
        box = (-5 * np.ones(n), 5 * np.ones(n)) if isinstance(s, A.LBFGSBSolver) else ()
        calls[0] = 0
        x = O.rosen_x0(n)
        with pytest.raises(KeyError, match="call 4"):
            s.minimize(A.DeviceObjective(fn), x, *box)
        assert s.last.status == L.E_USER and s.last.nfev == kth and ("evaluation %d" % kth) in s.last.msg
        assert np.all(np.isfinite(x)) and not np.array_equal(x, O.rosen_x0(n))  # the trial point in progress, as a functor's throw
        # the same object solves the next problem, as a fresh one does
        calls[0] = kth + 1
        x1, x2 = O.rosen_x0(n), O.rosen_x0(n)
        r1 = s.minimize(A.DeviceObjective(fn), x1, *box)
        r2 = make().minimize(A.DeviceObjective(inner), x2, *box)
        assert r1 == r2 and np.array_equal(x1, x2)


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR])
def test_non_finite_values_go_where_the_reference_sends_them(A, torch, ls):
    """a non-finite f is not an abort: the outcome -- the line search's own exception and text -- is the one the built-in
    objective produces when it overflows at the same points"""
    from lbfgspp_amd import _lib as L

    def outcome(f, x0):
        s = A.LBFGSSolver(A.LBFGSParam(max_iterations=20), linesearch=ls)
        x = x0.copy()
        try:
            return ("ok", repr(s.minimize(f, x)), s.last.nfev)
        except (RuntimeError, ArithmeticError, ValueError) as e:
            assert s.last.status != L.E_USER
            return (type(e).__name__, str(e), s.last.nfev)

    raised = 0
    for x0 in (np.full(10, 1e200), np.full(10, -3e76), O.rosen_x0(10) * 1e30):
        got = outcome(A.DeviceObjective(rosen_fn(torch)), x0)
        assert got == outcome(A.ExtendedRosenbrock(), x0), x0[0]
        raised += got[0] != "ok"
    assert raised >= 1
    # and a callback that turns to NaN in the middle of a search is never reported as the caller's abort: the search either
    # ends with its own exception or goes on, as the reference's does
    inner, calls = rosen_fn(torch), [0]

    def fn(x, g):
        calls[0] += 1
        f = inner(x, g)
        return float("nan") if calls[0] >= 3 else f
    s = A.LBFGSSolver(A.LBFGSParam(max_iterations=20), linesearch=ls)
    try:
        s.minimize(A.DeviceObjective(fn), O.rosen_x0(10))
    except (RuntimeError, ArithmeticError) as e:
        assert s.last.msg == str(e)
    assert s.last.status in (0, L.E_RUNTIME, L.E_LOGIC) and calls[0] == s.last.nfev >= 3


def test_autograd_objective_and_a_device_resident_x(A, torch):
    """from_autograd(0.5 |a x - b|^2) reaches the minimiser DiagQuadratic(a, b) reaches, to epsilon; x as a torch tensor on the
    device is updated in place"""
    n, eps = 4000, 1e-6
    a, b = O.quad_problem(n, 10.0, 3)
    par = A.LBFGSParam(m=8, epsilon=eps, epsilon_rel=0.0, max_iterations=200)
    xb = np.zeros(n)
    A.LBFGSSolver(par, linesearch=A.LS_MORE_THUENTE).minimize(A.DiagQuadratic(a, b), xb)
    at, bt = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(b, device="cuda:0")
    f = A.DeviceObjective.from_autograd(lambda x: 0.5 * ((at * x - bt) ** 2).sum())
    xt = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    s = A.LBFGSSolver(par, linesearch=A.LS_MORE_THUENTE)
    niter, fx = s.minimize(f, xt)
    x = xt.cpu().numpy()
    assert niter < 200 and s.final_grad_norm() <= eps
    # |a (x - x*)| = |grad| <= eps on both sides, a >= 1
    assert np.abs(x - xb).max() <= 2 * eps and np.abs(x - b / a).max() <= eps
    xn = np.zeros(n)
    assert s.minimize(f, xn) == (niter, fx) and np.array_equal(xn, x)  # host x and device x: the same solve


def test_a_problem_the_built_ins_cannot_express(A, torch):
    """ridge-regularised dense least squares, n = 1500 unknowns and 3000 rows: first-order condition recomputed on the host in
    float64; with a box: the projected-gradient condition (LBFGSB.h:141-151)"""
    rng = np.random.default_rng(5)
    rows, n, lam, eps = 3000, 1500, 0.1, 1e-6
    M = rng.standard_normal((rows, n)) / np.sqrt(rows)
    y = rng.standard_normal(rows)
    Mt, yt = torch.as_tensor(M, device="cuda:0"), torch.as_tensor(y, device="cuda:0")

    def fn(x, g):
        r = Mt @ x - yt
        torch.addmv(x, Mt.T, r, beta=lam, out=g)
        return 0.5 * float(r @ r) + 0.5 * lam * float(x @ x)

    def host_grad(x):
        return M.T @ (M @ x - y) + lam * x

    s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, max_iterations=500), linesearch=A.LS_MORE_THUENTE)
    x = np.zeros(n)
    niter, fx = s.minimize(A.DeviceObjective(fn), x)
    assert niter < 500
    assert np.linalg.norm(host_grad(x)) <= eps * max(1.0, np.linalg.norm(x))
    assert abs(fx - (0.5 * np.sum((M @ x - y) ** 2) + 0.5 * lam * x @ x)) <= 1e-12 * abs(fx)

    lb, ub = -0.05 * np.ones(n), 0.05 * np.ones(n)
    sb = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=0.0, past=0, max_iterations=500))
    xb = np.zeros(n)
    niter, fxb = sb.minimize(A.DeviceObjective(fn), xb, lb, ub)
    assert niter < 500 and np.all(xb >= lb) and np.all(xb <= ub) and np.any(np.abs(xb) == 0.05) and fxb >= fx
    assert np.abs(np.clip(xb - host_grad(xb), lb, ub) - xb).max() <= eps


def test_solver_extensions_with_a_callback(A, torch):
    """set_recursion applies to a callback as to any objective (the C++ path runs a device functor through either form);
    set_devices row-shards built-in objectives only, and says so (LBFGSX_E_INVALID), as LBFGSSolver::minimize does for a functor"""
    from lbfgspp_amd import _lib as L
    n = 4096
    a, b = O.quad_problem(n, 10.0, 2)
    par = A.LBFGSParam(m=6, epsilon=1e-8, epsilon_rel=0.0, max_iterations=200)
    f = A.DeviceObjective(quad_fn(torch, a, b))
    s = A.LBFGSSolver(par, linesearch=A.LS_MORE_THUENTE)
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    x = np.zeros(n)
    niter, _ = s.minimize(f, x)
    assert niter < 200 and np.abs(x - b / a).max() <= 1e-8
    s.set_devices([0, 0])
    calls = []
    with pytest.raises(ValueError, match="set_devices"):
        s.minimize(A.DeviceObjective(lambda xx, g: calls.append(1) or 0.0), np.zeros(n))
    assert s.last.status == L.E_INVALID and calls == []
    s.set_devices([])
    x2 = np.zeros(n)
    assert s.minimize(f, x2)[0] == niter and np.array_equal(x, x2)
