"""-m gpu: chain objectives (lbfgspp_amd.ChainObjective, csrc/chain_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/chain_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * the extended Rosenbrock function written as a chain follows the built-in bit for bit through whole solves;
  * the chained Rosenbrock function follows the reference (tests/golden/chain_golden.json), from Python and from C++;
  * a K = 3 problem converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import chain_ref as CR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _assert_same_bits, _counters, _solve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
BODY = {2: CR.ASYM2, 3: CR.ASYM3}
TERMS = {2: CR.asym2_terms, 3: CR.asym3_terms}
# the capped grid is 1024 blocks and a tile of the trial kernels 1024 packs: past 1024 tiles every block walks its stride twice
WRAP_F64 = 1024 * 1024 * 2 + 2 * 1024 * 2 + 3
WRAP_F32 = 1024 * 1024 * 4 + 2 * 1024 * 4 + 3  # the same with W = 4: two tiles past the wrap and a tail


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


def _shapes():
    ps = []
    for dtype in (O.F64, O.F32):
        for K in (2, 3):
            ns = [K, K + 1, 5, 127, 128, 129, 255, 256, 257, 511, 513, 1025, 2049, 4099, 3 * 4096 + 5]
            if dtype == O.F64:
                ns.append(WRAP_F64)
            elif K == 2:
                ns.append(WRAP_F32)
            for n in ns:
                ps.append(pytest.param(dtype, K, n, id="%s-K%d-%d" % ("f64" if dtype == O.F64 else "f32", K, n)))
    return ps


_compiled = {}


def _bind(c, K, rng):
    """compiles (once per process) and binds the statement tests' body with random per-term weights; returns (id, x -> (g, terms))"""
    L, n, dt = c.L, c.n, c.dt
    key = (K, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_chain(C.byref(h), c.dtype, K, BODY[K].encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    p0 = (0.5 + rng.random(n)).astype(dt)
    ptrs = (C.c_void_p * 4)()
    dev = C.c_void_p()
    L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(*(CR.ASYM_SCALARS + (0.0,) * 6))
    oid = C.c_int(-1)
    L.check(c.core.lbfgsx_objective_bind(c.h, _compiled[key], C.byref(ptrs), C.byref(cs), C.byref(oid)))
    assert oid.value == L.OBJ_BOUND

    def ref(x):
        tg, v = TERMS[K](x, p0)
        return CR.chain_grad(tg, n), v
    return oid.value, ref


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,K,n", _shapes())
def test_eval_statement(A, dtype, K, n):
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, K, rng)
        x = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, x)
        fx, g2, x2 = _d(3)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        g = c.down(L.VEC_G)
    g_ref, terms = ref(x)
    _bits(g, g_ref, "g")
    _sum_ok(fx.value, terms, dt, "f")
    _dot_ok(g2.value, g_ref, g_ref, dt, "g.g")
    _dot_ok(x2.value, x, x, dt, "x.x")


@pytest.mark.parametrize("dtype,K,n", _shapes())
def test_trial_statement_in_both_tile_orders(A, dtype, K, n):
    rng = np.random.default_rng(200 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, K, rng)
        xp = rng.standard_normal(n).astype(dt)
        d = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, xp)
        c.up(L.VEC_D, d)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        stale = np.full(n, -77.0, dt)
        step = 0.37
        xt_ref = R.axpy_ref(xp, d, step)
        g_ref, terms = ref(xt_ref)
        runs = []
        for k in range(2):
            c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible
            c.up(L.VEC_GT, stale)
            fx, dg = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
            assert _launches(c.core) == before + 1
            xt, gt = c.down(L.VEC_XT), c.down(L.VEC_GT)
            _bits(xt, xt_ref, "launch %d: x trial" % k)
            _bits(gt, g_ref, "launch %d: g trial" % k)
            runs.append((fx.value, dg.value))
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")
    assert runs[0] == runs[1], "f or g.d depends on the tile order"
    _sum_ok(runs[0][0], terms, dt, "f")
    _dot_ok(runs[0][1], g_ref, d, dt, "g.d")


@pytest.mark.parametrize("dtype,K,n", _shapes())
def test_b_eval_statement(A, dtype, K, n):
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, K, rng)
        x, _, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        c.up(L.VEC_X, x)
        c.up(L.VEC_LB, lb)
        c.up(L.VEC_UB, ub)
        fx, pg, x2 = _d(3)
        L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
        g = c.down(L.VEC_G)
    g_ref, terms = ref(x)
    _bits(g, g_ref, "g")
    _sum_ok(fx.value, terms, dt, "f")
    _dot_ok(x2.value, x, x, dt, "x.x")
    assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub)


@pytest.mark.parametrize("dtype,K,n", _shapes())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, K, n):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, K, rng)
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        for which, arr in ((L.VEC_X, x), (L.VEC_G, g0), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
            c.up(which, arr)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        step0 = 0.37
        runs0, hits0 = _ahead(c)
        dg, sm = _d(2)
        L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
        assert _ahead(c) == (runs0 + 1, hits0), "the fused kernel did not run"
        xt_ref = R.axpy_ref(x, d, step0)
        g_ref, terms = ref(xt_ref)
        _bits(c.down(L.VEC_XT), xt_ref, "x trial left by the fused pass")
        _bits(c.down(L.VEC_GT), g_ref, "g trial left by the fused pass")
        fx, dgt = _d(2)
        before = _launches(c.core)
        L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
        assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)
        _bits(c.down(L.VEC_G), g0, "g at xp is left alone")
    _dot_ok(dg.value, g0, d, dt, "g.d")
    assert sm.value == R.step_max_ref(x, d, lb, ub)
    _sum_ok(fx.value, terms, dt, "f")
    _dot_ok(dgt.value, g_ref, d, dt, "grad(x).d")


# ---------------------------------------------------------------- the extended Rosenbrock function as a chain
def _mask(n, dt):
    p0 = np.zeros(n, dt)
    p0[0::2] = 1
    return p0


@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("n", [2, 4096 + 2, 1_000_002])
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR])
def test_masked_chain_is_the_builtin_extended_rosenbrock(A, ls, dtype, n, m):
    dt = NPDT[dtype]
    x0 = O.rosen_x0(n, 7, dtype)
    p = dict(m=m, max_iterations=25)
    builtin = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt), A.ExtendedRosenbrock(), x0)
    chain = _solve(A, A.LBFGSSolver(A.LBFGSParam(**p), linesearch=ls, dtype=dt),
                   A.ChainObjective(CR.ROSEN_MASKED, K=2, data=(_mask(n, dt),)), x0)
    assert builtin["nfev"] >= 1 and builtin["count"] == builtin["nfev"]
    _assert_same_bits(builtin, chain)


@pytest.mark.parametrize("m", [3, 10])
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
def test_masked_chain_is_the_builtin_under_lbfgsb(A, dtype, m):
    dt = NPDT[dtype]
    n = 20000
    x0 = O.rosen_x0(n, 7, dtype)
    lb, ub = np.full(n, -0.5, dt), np.full(n, 0.9, dt)
    prm = dict(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=30)
    s1, s2 = A.LBFGSBSolver(A.LBFGSBParam(**prm), dtype=dt), A.LBFGSBSolver(A.LBFGSBParam(**prm), dtype=dt)
    builtin = _solve(A, s1, A.ExtendedRosenbrock(), x0, (lb, ub))
    chain = _solve(A, s2, A.ChainObjective(CR.ROSEN_MASKED, K=2, data=(_mask(n, dt),)), x0, (lb, ub))
    _assert_same_bits(builtin, chain)
    st1, st2 = s1.stats(), s2.stats()
    assert (st1["gcp_crossings"], st1["submin_sweeps"]) == (st2["gcp_crossings"], st2["submin_sweeps"])


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "chain_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g["instances"]


def _start(n):
    """tests/cpp/chain_probe.cpp: start()"""
    t = np.arange(n, dtype=np.float64) * 0.61803398874989485
    return -0.4 + 0.4 * (t - np.floor(t))


@pytest.mark.parametrize("inst", _golden(), ids=lambda i: "%s-%d" % (i["solver"], i["n"]))
def test_chained_rosenbrock_follows_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(n)
        f = A.ChainObjective(CR.CHAINED_ROSEN, K=2)
        if inst["solver"] == "lbfgs":
            s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
            niter, fx = s.minimize(f, x)
        else:
            s = A.LBFGSBSolver(A.LBFGSBParam(past=0, **prm))
            niter, fx = s.minimize(f, x, np.full(n, inst["lb"]), np.full(n, inst["ub"]))
        x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
        dx, df = float(np.abs(x - x_ref).max()), abs(fx - inst["f"][k - 1])
        print("k %d: niter %d nfev %d |dx| %.3g |df| %.3g" % (k, niter, s.last.nfev, dx, df))
        assert (niter, s.last.nfev) == (inst["niter"][k - 1], inst["nfev"][k - 1])
        assert dx <= tol and df <= tol


def test_cpp_chain_objective_follows_the_reference(tmp_path):
    """tests/cpp/chain_probe.cpp with ChainObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "chain_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DCHAIN_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "chain_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()
    for n in sorted({i["n"] for i in insts}):
        kmax = max(i["iterations"] for i in insts if i["n"] == n)
        out = subprocess.run([exe, str(n), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "CHAIN PROBE OK" in out.stdout, out.stdout[-2000:]
        rows = {}
        for line in out.stdout.splitlines():
            w = line.split()
            if w and w[0] in ("lbfgs", "lbfgsb"):
                rows[(w[0], int(w[1]))] = (int(w[2]), float(w[4]), np.array([float(v) for v in w[5:]]))
        for inst in (i for i in insts if i["n"] == n):
            for k in range(1, inst["iterations"] + 1):
                niter, fx, x = rows[(inst["solver"], k)]
                x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
                assert niter == inst["niter"][k - 1]
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], n, k)


# ---------------------------------------------------------------- convergence, K = 3
def _smoothing_instance(n=20_001):
    rng = np.random.default_rng(2026)
    t = np.linspace(0.0, 1.0, n)
    return 1.0 + rng.random(n), np.sin(6.0 * t) + 0.05 * rng.standard_normal(n), 2.0


def _smoothing_grad(x, p0, p1, c0):
    """the gradient in double, written independently of the body: 2 p0 (x - p1) on the coordinates a term starts at, plus
    2 c0 D'D x for the second-difference operator D"""
    n = x.size
    g = np.zeros(n)
    g[:n - 2] = 2.0 * p0[:n - 2] * (x[:n - 2] - p1[:n - 2])
    s = x[:-2] - 2.0 * x[1:-1] + x[2:]
    g[:-2] += 2.0 * c0 * s
    g[1:-1] -= 4.0 * c0 * s
    g[2:] += 2.0 * c0 * s
    return g


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_second_difference_smoothing_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    p0, p1, c0 = _smoothing_instance()
    n, eps, cap = p0.size, 1e-6, 2000
    f = A.ChainObjective(CR.SECOND_DIFF, K=3, data=(p0, p1), scalars=(c0,))
    x = np.zeros(n)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(_smoothing_grad(x, p0, p1, c0)))
    else:
        lb, ub = np.full(n, -0.8), np.full(n, 0.8)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        niter, fx = s.minimize(f, x, lb, ub)
        g = _smoothing_grad(x, p0, p1, c0)
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.any(x == 0.8) and np.any(x == -0.8)  # sin(6 t) + noise leaves the box: bounds are active
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    print("%s: niter %d nfev %d fx %.9g stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, measure, bound))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound


# ---------------------------------------------------------------- launch accounting
def test_chain_solve_issues_the_launches_of_the_builtin(A):
    core, _ = A.load()
    n, m, iters = 200_000, 6, 20
    x0 = O.rosen_x0(n)
    prm = dict(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters)
    out = {}
    for name, f in (("builtin", A.ExtendedRosenbrock()), ("chain", A.ChainObjective(CR.ROSEN_MASKED, K=2, data=(_mask(n, np.float64),)))):
        s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x)
        c1 = _counters(core)
        out[name] = (niter, s.last.nfev, c1[0] - c0[0])
    print(out)
    assert out["chain"] == out["builtin"] and out["chain"][2] > 0


def test_lbfgsb_chain_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    n, m, iters = 20000, 6, 25
    x0 = O.rosen_x0(n)
    lb, ub = np.full(n, -0.5), np.full(n, 0.9)
    out = {}
    for name, f in (("builtin", A.ExtendedRosenbrock()), ("chain", A.ChainObjective(CR.ROSEN_MASKED, K=2, data=(_mask(n, np.float64),)))):
        s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        s.minimize(f, x, lb, ub)
        c1 = _counters(core)
        ahead = (C.c_int64 * 2)()
        assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
        out[name] = (c1[0] - c0[0], ahead[0], ahead[1])
    print(out)
    assert out["chain"][1] > 0 and out["chain"][2] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["chain"] == out["builtin"]


# ---------------------------------------------------------------- refusals
def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    core, _ = A.load()
    f = A.ChainObjective(CR.CHAINED_ROSEN, K=2)
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, _start(1000))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, _start(1000))
    batch = B.LockstepBatch(A.LBFGSParam(m=3, max_iterations=3), 64, 2, dtype=np.float64)
    try:
        for obj in (f, A.TermObjective(CR.CHAINED_ROSEN, K=2)):  # the same refusal for both
            with pytest.raises(TypeError, match="fn must be callable"):
                batch.minimize_fn(obj, np.zeros((2, 64)))
    finally:
        batch.close()
    # n < K: binding to a context is refused by the library itself
    with Ctx(A, O.F64, 2) as c:
        h3 = A.ChainObjective(CR.SECOND_DIFF, K=3)
        oid = C.c_int(-1)
        assert core.lbfgsx_objective_bind(c.h, h3.compile(), None, None, C.byref(oid)) == L.E_INVALID
        assert "n = 2 is less than K = 3" in L.last_error()
    with pytest.raises(ValueError, match="n = 1 is less than K = 2"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(1))
