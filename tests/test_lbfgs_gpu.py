"""-m gpu: parity of the HIP path (through the C ABI) against the CPU oracle on identical inputs."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

TOL = {O.F64: 1e-10, O.F32: 1e-4}  # BASELINE.json north_star tolerances (iterate parity)


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


class Ctx:
    def __init__(self, A, dtype, n, m, flags=0):
        from lbfgspp_amd import _lib as L
        self.L = L
        self.core, _ = A.load()
        self.h = C.c_void_p()
        L.check(self.core.lbfgsx_create(C.byref(self.h), dtype, n, m, 0, flags))
        self.n, self.dt = n, O.NPDT[dtype]

    def up(self, which, arr):
        arr = np.ascontiguousarray(arr, self.dt)
        self.L.check(self.core.lbfgsx_upload(self.h, which, arr.ctypes.data_as(C.c_void_p)))

    def down(self, which):
        out = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        self.core.lbfgsx_destroy(self.h)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("n,m,npairs", [(1000, 6, 0), (1000, 6, 3), (4099, 6, 6), (4099, 5, 13), (65537, 10, 10),
                                        (2, 3, 2), (7, 3, 5), (3001, 32, 35), (3001, 33, 33), (2050, 70, 75),
                                        (1030, 128, 131), (1030, 129, 133), (515, 200, 60)])  # around the persistent launch's column list (128)
def test_apply_Hv_matches_oracle(A, oracle, dtype, n, m, npairs):
    rng = np.random.default_rng(1234 + n + npairs)
    dt = O.NPDT[dtype]
    S = rng.standard_normal((max(npairs, 1), n)).astype(dt)
    # y = s scaled + noise keeps s.y > 0 like a real curvature pair
    Y = (S * (1.0 + rng.random((max(npairs, 1), n))) + 0.05 * rng.standard_normal((max(npairs, 1), n))).astype(dt)
    S, Y = S[:npairs], Y[:npairs]
    v = rng.standard_normal(n).astype(dt)
    ref = oracle.apply_Hv(dtype, m, S.reshape(npairs, n), Y.reshape(npairs, n), v, -1.0)

    c = Ctx(A, dtype, n, m)
    L = c.L
    for k in range(npairs):
        L.check(c.core.lbfgsx_bfgs_add_correction_host(c.h, S[k].ctypes.data_as(C.c_void_p),
                                                      Y[k].ctypes.data_as(C.c_void_p)))
    assert c.core.lbfgsx_bfgs_ncorr(c.h) == min(npairs, m)
    c.up(L.VEC_G, v)
    dg = C.c_double()
    L.check(c.core.lbfgsx_apply_Hv(c.h, L.VEC_G, -1.0, C.byref(dg)))
    got = c.down(L.VEC_D)
    c.close()
    scale = np.abs(ref).max() + 1e-300
    eps = np.finfo(dt).eps
    assert np.abs(got - ref).max() <= 4 * eps * scale, "two-loop recursion deviates from the oracle"
    # the oracle equals the exact reference on these inputs, every element (tests/test_twoloop_ref_cpu.py), and no exact dot
    # lies near a rounding boundary: the product is held to the exact reference, every element
    import twoloop_ref as T
    Sr, Yr, ptr = T.ring_fill([(S[k], Y[k]) for k in range(npairs)], m)
    exact = T.two_loop(Sr, Yr, ptr, m, v, -1.0, None, dt)
    assert not exact.ambiguous
    assert np.array_equal(got, exact.d) and np.array_equal(ref, exact.d)
    assert dg.value == exact.dg
    # fused dg = v . d
    want = float(np.dot(v.astype(np.float64), got.astype(np.float64)))
    assert abs(dg.value - want) <= 1e-5 * abs(want) + 1e-30 if dtype == O.F32 else abs(dg.value - want) <= 1e-12 * abs(want) + 1e-300


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("obj,n", [(O.OBJ_QUAD, 5001), (O.OBJ_ROSEN, 5002), (O.OBJ_ROSEN, 2), (O.OBJ_QUAD, 1)])
def test_eval_matches_oracle(A, oracle, dtype, obj, n):
    dt = O.NPDT[dtype]
    rng = np.random.default_rng(7 + n)
    x = rng.standard_normal(n).astype(dt)
    a, b = O.quad_problem(n, dtype=dtype) if obj == O.OBJ_QUAD else (None, None)
    fx_ref, g_ref = oracle.eval(dtype, obj, x, a, b)
    c = Ctx(A, dtype, n, 3)
    L = c.L
    c.up(L.VEC_X, x)
    if a is not None:
        c.up(L.VEC_A, a)
        c.up(L.VEC_B, b)
    fx, g2, x2 = C.c_double(), C.c_double(), C.c_double()
    L.check(c.core.lbfgsx_eval(c.h, obj, C.byref(fx), C.byref(g2), C.byref(x2)))
    g = c.down(L.VEC_G)
    c.close()
    assert np.array_equal(g, g_ref), "gradient is element-wise: must be bit-exact"
    assert fx.value == fx_ref, "objective sum must round identically"
    assert g2.value == float(dt(np.sum(g.astype(np.longdouble) ** 2))) or abs(g2.value - float(np.sum(g.astype(np.float64) ** 2))) <= 4 * np.finfo(dt).eps * g2.value


def test_device_generators_match_host_spec(A):
    n = 10007
    c = Ctx(A, O.F64, n, 3)
    L = c.L
    L.check(c.core.lbfgsx_gen_diag_quad(c.h, 10.0, 1))
    L.check(c.core.lbfgsx_gen_rosen_x0(c.h, 7))
    a, b = O.quad_problem(n, 10.0, 1)
    assert np.array_equal(c.down(L.VEC_A), a) and np.array_equal(c.down(L.VEC_B), b)
    assert np.array_equal(c.down(L.VEC_X), O.rosen_x0(n, 7))
    c.close()


def _trajectory(A, oracle, dtype, ls, obj, n, m, iters, x0, a=None, b=None, **pk):
    p = O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters, **pk)
    tr_ref = O.TraceBuf(n, cap=1024)
    x_ref, r_ref = oracle.lbfgs(dtype, ls, obj, x0, p, a=a, b=b, trace=tr_ref)
    par = A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters, **pk)
    s = A.LBFGSSolver(par, linesearch=ls, dtype=O.NPDT[dtype])
    tr = A.TraceBuffer(n, cap=1024)
    x = np.array(x0, dtype=O.NPDT[dtype])
    f = A.DiagQuadratic(a, b) if obj == O.OBJ_QUAD else A.ExtendedRosenbrock()
    status = 0
    try:
        niter, fx = s.minimize(f, x, trace=tr)
    except (RuntimeError, ArithmeticError, ValueError):
        status = 1
        niter, fx = s.last.niter, s.last.fx
    return dict(x=x, niter=niter, fx=fx, tr=tr, nfev=s.last.nfev, status=status, msg=s.last.msg,
                x_ref=x_ref, r_ref=r_ref, tr_ref=tr_ref)


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT, O.LS_BT, O.LS_BR])
def test_trajectory_quadratic_f64(A, oracle, ls):
    n = 20000
    a, b = O.quad_problem(n)
    r = _trajectory(A, oracle, O.F64, ls, O.OBJ_QUAD, n, 10, 40, np.zeros(n), a, b)
    assert r["status"] == 0 and r["r_ref"].status == 0
    assert (r["niter"], r["nfev"]) == (r["r_ref"].niter, r["r_ref"].nfev)
    k = r["tr_ref"].count
    assert r["tr"].count == k
    assert np.abs(r["tr"].xs[:k] - r["tr_ref"].xs[:k]).max() <= TOL[O.F64]
    assert np.abs(r["x"] - r["x_ref"]).max() <= TOL[O.F64]
    assert np.allclose(r["tr"].fx[:k], r["tr_ref"].fx[:k], rtol=1e-13, atol=0)


@pytest.mark.parametrize("ls", [O.LS_NW, O.LS_MT])
@pytest.mark.parametrize("n,m,iters", [(20000, 10, 60), (200000, 20, 30), (6000, 40, 55),
                                       (3000, 140, 160)])  # a history longer than the persistent launch's column list: step launches
def test_trajectory_rosenbrock_f64(A, oracle, ls, n, m, iters):
    r = _trajectory(A, oracle, O.F64, ls, O.OBJ_ROSEN, n, m, iters, O.rosen_x0(n))
    assert r["status"] == r["r_ref"].status == 0
    assert (r["niter"], r["nfev"]) == (r["r_ref"].niter, r["r_ref"].nfev)
    k = r["tr_ref"].count
    # iterate-for-iterate: every evaluated point within 1e-10 of the reference's
    assert np.abs(r["tr"].xs[:k] - r["tr_ref"].xs[:k]).max() <= TOL[O.F64]
    assert np.abs(r["x"] - r["x_ref"]).max() <= TOL[O.F64]


def test_trajectory_rosenbrock_f32(A, oracle):
    n = 100000
    r = _trajectory(A, oracle, O.F32, O.LS_MT, O.OBJ_ROSEN, n, 10, 30, O.rosen_x0(n, 1000, O.F32))
    assert (r["niter"], r["nfev"]) == (r["r_ref"].niter, r["r_ref"].nfev)
    k = r["tr_ref"].count
    assert np.abs(r["tr"].xs[:k] - r["tr_ref"].xs[:k]).max() <= TOL[O.F32]
    assert np.abs(r["x"].astype(np.float64) - r["x_ref"].astype(np.float64)).max() <= TOL[O.F32]


def test_readme_rosenbrock_known_answers(A):
    """Rosenbrock n=10, f64, epsilon=1e-6, max_iterations=100 (reference README.md:60-95)."""
    expect = {O.LS_NW: (22, 36), O.LS_MT: (21, 28), O.LS_BT: (22, 31), O.LS_BR: (22, 31)}
    for ls, (nit, nfev) in expect.items():
        s = A.LBFGSSolver(A.LBFGSParam(epsilon=1e-6, max_iterations=100), linesearch=ls)
        x = np.zeros(10)
        niter, fx = s.minimize(A.ExtendedRosenbrock(), x)
        assert (niter, s.last.nfev) == (nit, nfev)
        assert np.abs(x - 1.0).max() < 1e-4
    s = A.LBFGSSolver(A.LBFGSParam(epsilon=1e-6, epsilon_rel=0.0, max_iterations=100))
    x = np.zeros(10)
    niter, fx = s.minimize(A.ExtendedRosenbrock(), x)
    assert niter == 23 and fx < 1e-18  # the README transcript: "23 iterations"


def test_example_rosenbrock_float(A, oracle):
    """reference examples/example-rosenbrock.cpp: LBFGSParam<float>, n=10, x0=0."""
    p = O.lbfgs_params()
    x_ref, r_ref = oracle.lbfgs(O.F32, O.LS_NW, O.OBJ_ROSEN, np.zeros(10, np.float32), p)
    s = A.LBFGSSolver(A.LBFGSParam(), dtype=np.float32)
    x = np.zeros(10, np.float32)
    try:
        niter, fx = s.minimize(A.ExtendedRosenbrock(), x)
        status = 0
    except RuntimeError:
        status, niter = 3, s.last.niter
    assert (status != 0) == (r_ref.status != 0)
    if status == 0:
        assert niter == r_ref.niter and np.abs(x - x_ref).max() <= 1e-4


def test_errors_map_to_reference_exceptions(A):
    with pytest.raises(ValueError, match="'m' must be positive"):
        A.LBFGSSolver(A.LBFGSParam(m=0))
    with pytest.raises(ValueError, match="'wolfe' must satisfy ftol < wolfe < 1"):
        A.LBFGSSolver(A.LBFGSParam(wolfe=1.5))
    # NocedalWright refuses a non-strong-Wolfe termination condition (reference NocedalWright.h:95-96)
    s = A.LBFGSSolver(A.LBFGSParam(linesearch=1), linesearch=O.LS_NW)
    with pytest.raises(ValueError, match="LBFGS_LINESEARCH_BACKTRACKING_STRONG_WOLFE"):
        s.minimize(A.ExtendedRosenbrock(), np.zeros(10))


def test_large_n_properties(A):
    """Full-size style checks that do not need the oracle: determinism and H-linearity at n = 2^24."""
    n, m = 1 << 24, 10
    par = A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=12)
    s = A.LBFGSSolver(par, linesearch=O.LS_MT)
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    fxs = []
    for rep in range(2):
        h = s.prepare(n)
        L.check(core.lbfgsx_gen_rosen_x0(h, 7))
        niter, fx = s.minimize_resident(A.ExtendedRosenbrock(), n)
        fxs.append((niter, s.last.nfev, fx, s.last.gnorm))
    assert fxs[0] == fxs[1], "run-to-run results must be bit-reproducible"
    # linearity of v -> H v with the final history: H(2v) == 2 H(v) exactly (scaling by 2 is exact)
    h = s.ctx
    dg1, dg2 = C.c_double(), C.c_double()
    L.check(core.lbfgsx_apply_Hv(h, L.VEC_G, -1.0, C.byref(dg1)))
    g1 = np.empty(n // 4096)
    L.check(core.lbfgsx_gather(h, L.VEC_D, 4096, g1.ctypes.data_as(C.POINTER(C.c_double))))
    L.check(core.lbfgsx_apply_Hv(h, L.VEC_G, -2.0, C.byref(dg2)))
    g2 = np.empty(n // 4096)
    L.check(core.lbfgsx_gather(h, L.VEC_D, 4096, g2.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.array_equal(2.0 * g1, g2) and dg2.value == 2.0 * dg1.value
    assert dg1.value < 0  # -H g is a descent direction


# ---------------------------------------------------------------- golden fixtures (need no oracle library)
import golden_util as G  # noqa: E402

_GOLD = G.load("lbfgs_golden.json")


@pytest.mark.parametrize("case", _GOLD["cases"], ids=[c["name"] for c in _GOLD["cases"]])
def test_lbfgs_golden(A, case):
    x0, a, b = G.case_inputs(case)
    pr = case["params"]
    par = A.LBFGSParam(**{k: pr[k] for k in ("m", "epsilon", "epsilon_rel", "past", "delta", "max_iterations",
                                             "linesearch", "max_linesearch", "min_step", "max_step", "ftol", "wolfe")})
    s = A.LBFGSSolver(par, linesearch=case["ls"], dtype=O.NPDT[case["dtype"]])
    tr = A.TraceBuffer(case["n"], cap=1024, stride=case["stride"])
    x = x0.copy()
    f = A.DiagQuadratic(a, b) if case["obj"] == O.OBJ_QUAD else A.ExtendedRosenbrock()
    niter, fx = s.minimize(f, x, trace=tr)
    assert (niter, s.last.nfev) == (case["niter"], case["nfev"])
    k = tr.count
    tol = TOL[case["dtype"]]
    assert np.abs(tr.xs[:k].ravel() - G.unhex(case["trace_xs"])).max() <= tol
    assert np.abs(np.asarray(x[::case["stride"]], np.float64) - G.unhex(case["x_sample"])).max() <= tol
    # with order-independent reductions the HIP path is expected to reproduce the reference bit for bit
    assert fx == float.fromhex(case["fx"])


@pytest.mark.parametrize("dtype,n,m", [(O.F64, 300002, 7), (O.F32, 100002, 5), (O.F64, 2048, 12)])
def test_persistent_two_loop_is_bit_identical(A, oracle, monkeypatch, dtype, n, m):
    """k_twoloop_persist (one launch per apply_Hv, part of q resident on the CUs) against the 2c+1 step launches and
    against the oracle; its use is asserted through lbfgsx_persistent_launches."""
    import ctypes as C
    import gc
    core, _ = A.load()
    core.lbfgsx_persistent_launches.restype = C.c_int64
    core.lbfgsx_persistent_launches.argtypes = [C.c_void_p]
    x0 = O.rosen_x0(n, 11, dtype)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LBFGSX_PERSIST", mode)
        gc.collect()
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=2 * m + 5),
                          linesearch=A.LS_MORE_THUENTE, dtype=O.NPDT[dtype])
        x = x0.copy()
        niter, fx = s.minimize(A.ExtendedRosenbrock(), x)
        res[mode] = (niter, s.last.nfev, fx, x, int(core.lbfgsx_persistent_launches(s.ctx() if callable(s.ctx) else s.ctx)))
        del s
        gc.collect()
    assert res["1"][4] > 0 and res["0"][4] == 0
    assert res["1"][:3] == res["0"][:3] and np.array_equal(res["1"][3], res["0"][3])
    x_ref, r = oracle.lbfgs(dtype, O.LS_MT, O.OBJ_ROSEN, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0,
                                                                            max_iterations=2 * m + 5))
    assert (r.niter, r.nfev) == res["1"][:2] and np.array_equal(res["1"][3], x_ref)


@pytest.mark.parametrize("dtype,n,m,ls", [(O.F64, 1000, 6, O.LS_MT), (O.F32, 2050, 5, O.LS_MT), (O.F64, 4094, 10, O.LS_NW),
                                          (O.F64, 4096, 10, O.LS_NW)])
def test_default_switch_between_the_step_launches_and_the_persistent_kernel(A, oracle, monkeypatch, dtype, n, m, ls):
    """The PRODUCT's default: below LBFGSX_PERSIST_MIN_N = 4096 elements apply_Hv is the 2c+1 step launches, from there on the
    persistent kernel (tests/conftest.py lifts the threshold for the rest of the suite).  With the environment variable
    removed the switch must sit exactly there, and both forms must give the bits of the other and of the oracle."""
    import ctypes as C
    import gc
    core, _ = A.load()
    core.lbfgsx_persistent_launches.restype = C.c_int64
    core.lbfgsx_persistent_launches.argtypes = [C.c_void_p]
    obj, oobj = (A.ExtendedRosenbrock(), O.OBJ_ROSEN) if ls == O.LS_MT else (None, O.OBJ_QUAD)
    a = b = None
    if obj is None:
        a, b = O.quad_problem(n, 10.0, 1, dtype)
        obj = A.DiagQuadratic(a, b)
    x0 = O.rosen_x0(n + (n % 2), 11, dtype)[:n] if ls == O.LS_MT else np.zeros(n, O.NPDT[dtype])
    if ls == O.LS_MT and n % 2:
        pytest.skip("the extended Rosenbrock objective needs an even n")
    res = {}
    for mode in ("default", "lifted"):
        if mode == "default":
            monkeypatch.delenv("LBFGSX_PERSIST_MIN_N", raising=False)
        else:
            monkeypatch.setenv("LBFGSX_PERSIST_MIN_N", "0")
        gc.collect()
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=2 * m + 5), linesearch=ls, dtype=O.NPDT[dtype])
        x = x0.copy()
        niter, fx = s.minimize(obj, x)
        res[mode] = (niter, s.last.nfev, fx, x, int(core.lbfgsx_persistent_launches(s.ctx)))
        del s
        gc.collect()
    assert res["lifted"][4] > 0
    assert (res["default"][4] == 0) == (n < 4096), "n = %d: %d persistent launches by default" % (n, res["default"][4])
    assert res["default"][:3] == res["lifted"][:3] and np.array_equal(res["default"][3], res["lifted"][3])
    x_ref, r = oracle.lbfgs(dtype, ls, oobj, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=2 * m + 5), a=a, b=b)
    assert (r.niter, r.nfev) == res["default"][:2] and np.array_equal(res["default"][3], x_ref)


@pytest.mark.parametrize("dtype,n,m,ls", [(O.F64, 300002, 7, O.LS_MT), (O.F32, 100002, 5, O.LS_MT), (O.F64, 2051, 12, O.LS_NW),
                                          (O.F64, 20_000_002, 4, O.LS_MT), (O.F64, 10_000_000, 10, O.LS_NW)])
def test_both_forms_of_the_meeting_points_give_the_same_bits(A, oracle, monkeypatch, dtype, n, m, ls):
    """Between two steps of the persistent launch the blocks meet.  Default (round 4): every block leaves its partial sums
    as tagged 16-byte words and moves on, block 0 polls them, adds them up and publishes {generation, dot} in one tagged
    word, which the others poll AFTER issuing the next step's first loads, keeping the dots in their own LDS table.
    LBFGSX_MEET=last (rounds 1-3): a ticket, the last block to arrive reduces, publishes the dot and a generation word the
    others wait for at the end of the step, and every block fetches the coefficient back.  Double-double partials, correctly
    rounded totals: the same trajectory bit for bit, with the post statements fused (step 0 of the launch, five sums) and
    without; n = 2e7 has a streamed part, n = 1e7 is cfg2's size (q fully resident), n = 2051 a scalar tail; the oracle
    pins both.  No launch may have timed out (a time-out is redone with the step launches: same bits, so only the counter
    shows it)."""
    import gc
    obj, oobj = (A.ExtendedRosenbrock(), O.OBJ_ROSEN) if ls == O.LS_MT else (None, O.OBJ_QUAD)
    a = b = None
    if obj is None:
        a, b = O.quad_problem(n, 10.0, 1, dtype)
        obj = A.DiagQuadratic(a, b)
    x0 = O.rosen_x0(n, 11, dtype) if ls == O.LS_MT else np.zeros(n, O.NPDT[dtype])
    iters = 2 * m + 6
    res = {}
    for meet, fuse in (("all", "1"), ("last", "1"), ("all", "0")):
        monkeypatch.setenv("LBFGSX_MEET", meet)
        monkeypatch.setenv("LBFGSX_FUSE_POST", fuse)
        gc.collect()
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters), linesearch=ls, dtype=O.NPDT[dtype])
        x = x0.copy()
        tr = A.TraceBuffer(n, cap=256, with_x=False)
        niter, fx = s.minimize(obj, x, trace=tr)
        res[(meet, fuse)] = (niter, s.last.nfev, fx, x, tr.fx[:tr.count].copy())
        import ctypes as C
        pc = (C.c_int64 * 4)()
        A.load()[0].lbfgsx_persist_counts(s.ctx, C.byref(pc))
        assert pc[0] >= iters - 1 and pc[1] == 0 and pc[3] == 0, (meet, fuse, tuple(pc))
        del s
        gc.collect()
    ref = res[("last", "1")]
    for k, r in res.items():
        assert r[:3] == ref[:3] and np.array_equal(r[3], ref[3]) and np.array_equal(r[4], ref[4]), k
    if n <= 300002:
        x_ref, rr = oracle.lbfgs(dtype, ls, oobj, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), a=a, b=b)
        assert (rr.niter, rr.nfev) == ref[:2] and np.array_equal(ref[3], x_ref)


def _spec_counts(A, s):
    import ctypes as C
    core, _ = A.load()
    out = (C.c_int64 * 3)()
    core.lbfgsx_spec_counts(s.ctx, C.byref(out))
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("dtype,n,m,ls", [(O.F64, 300002, 7, O.LS_MT), (O.F32, 100002, 5, O.LS_MT), (O.F64, 2051, 12, O.LS_NW),
                                          (O.F64, 20_000_002, 4, O.LS_MT)])
def test_post_statements_fused_into_the_recursion_launch_change_no_bit(A, oracle, monkeypatch, dtype, n, m, ls):
    """lbfgsx_post_linesearch_spec: K3 (s, y, the four sums) as step 0 of the persistent launch that speculatively
    computes the next direction.  Same trajectory, evaluation for evaluation, as the separate launches
    (LBFGSX_FUSE_POST=0) and as the oracle; n = 2051 has a scalar tail, n = 2e7 a streamed (non-resident) part."""
    odd = (n % 2) == 1     # an odd dimension (scalar tail in f64) needs the quadratic: the Rosenbrock pairs want n even
    a, b = O.quad_problem(n, 10.0, 1, dtype) if odd else (None, None)
    x0 = np.zeros(n, O.NPDT[dtype]) if odd else O.rosen_x0(n, 3, dtype)
    obj = O.OBJ_QUAD if odd else O.OBJ_ROSEN
    iters = 2 * m + 6 if n < 10_000_000 else 8
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LBFGSX_FUSE_POST", mode)
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters),
                          linesearch=A.LS_MORE_THUENTE if ls == O.LS_MT else A.LS_NOCEDAL_WRIGHT, dtype=O.NPDT[dtype])
        x = x0.copy()
        tr = A.TraceBuffer(n, cap=256, with_x=False)
        niter, fx = s.minimize(A.DiagQuadratic(a, b) if odd else A.ExtendedRosenbrock(), x, trace=tr)
        res[mode] = (niter, s.last.nfev, fx, x, tr.fx[:tr.count].copy(), _spec_counts(A, s))
        s.close()
    fused, used, rejected = res["1"][5]
    assert fused == iters and used == iters - 1 and rejected == 0   # the last iteration stops before using its direction
    assert res["0"][5] == (0, 0, 0)
    assert res["1"][:3] == res["0"][:3] and np.array_equal(res["1"][3], res["0"][3]) and np.array_equal(res["1"][4], res["0"][4])
    if n < 10_000_000:
        x_ref, r = oracle.lbfgs(dtype, ls, obj, x0, O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), a=a, b=b)
        assert (r.niter, r.nfev) == res["1"][:2] and np.array_equal(res["1"][3], x_ref)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("n,m,npairs,accept", [(70002, 6, 4, False), (70002, 6, 4, True), (4100, 5, 9, False), (1000, 4, 0, False),
                                              (1000, 4, 0, True), (300002, 5, 5, True)])
def test_fused_post_launch_statement_level(A, oracle, dtype, n, m, npairs, accept):
    """lbfgsx_post_linesearch_spec on hand-made points.  A pair with s.y <= eps y.y is rejected by the driver
    (LBFGS.h:161) and the recursion runs on the OLD history: the fused launch sees the same test fail, stops after the
    post statements, and lbfgsx_apply_Hv computes the direction the ordinary way.  An accepted pair: the direction of
    the fused launch is the one lbfgsx_apply_Hv hands out after the commit, equal to the oracle's product on the
    history that includes the new pair.  The four sums and the stored s, y are k_post's in both cases."""
    rng = np.random.default_rng(99 + n + npairs)
    dt = O.NPDT[dtype]
    S = rng.standard_normal((max(npairs, 1), n)).astype(dt)
    Y = (S * (1.0 + rng.random((max(npairs, 1), n))) + 0.05 * rng.standard_normal((max(npairs, 1), n))).astype(dt)
    S, Y = S[:npairs], Y[:npairs]
    xp, gp = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    s_new = rng.standard_normal(n).astype(dt)
    y_new = ((1.5 if accept else -1.5) * s_new + 0.05 * rng.standard_normal(n)).astype(dt)
    x, g = (xp + s_new).astype(dt), (gp + y_new).astype(dt)
    s_new, y_new = x - xp, g - gp      # what the statements will form
    c = Ctx(A, dtype, n, m)
    L = c.L
    for k in range(npairs):
        L.check(c.core.lbfgsx_bfgs_add_correction_host(c.h, S[k].ctypes.data_as(C.c_void_p), Y[k].ctypes.data_as(C.c_void_p)))
    c.up(L.VEC_X, xp)
    c.up(L.VEC_G, gp)
    L.check(c.core.lbfgsx_ls_begin(c.h))
    c.up(L.VEC_XT, x)
    c.up(L.VEC_GT, g)
    L.check(c.core.lbfgsx_ls_end(c.h, 0))
    r = [C.c_double() for _ in range(4)]
    L.check(c.core.lbfgsx_post_linesearch_spec(c.h, -1.0, *[C.byref(v) for v in r]))
    g2, x2, sy, yy = [v.value for v in r]
    f64 = np.float64
    for got, want in ((g2, np.dot(g.astype(f64), g.astype(f64))), (x2, np.dot(x.astype(f64), x.astype(f64))),
                      (sy, np.dot(s_new.astype(f64), y_new.astype(f64))), (yy, np.dot(y_new.astype(f64), y_new.astype(f64)))):
        assert abs(got - want) <= (1e-12 if dtype == O.F64 else 2e-6) * abs(want)
    assert (sy > np.finfo(dt).eps * yy) == accept
    counts = (C.c_int64 * 3)()
    c.core.lbfgsx_spec_counts(c.h, C.byref(counts))
    assert tuple(counts) == (1, 0, 0 if accept else 1)
    if accept:
        L.check(c.core.lbfgsx_commit_correction(c.h))
        hist_S, hist_Y = np.vstack([S.reshape(npairs, n), s_new[None]]), np.vstack([Y.reshape(npairs, n), y_new[None]])
    else:
        hist_S, hist_Y = S.reshape(npairs, n), Y.reshape(npairs, n)
    dg = C.c_double()
    L.check(c.core.lbfgsx_apply_Hv(c.h, L.VEC_G, -1.0, C.byref(dg)))
    got = c.down(L.VEC_D)
    c.core.lbfgsx_spec_counts(c.h, C.byref(counts))
    assert tuple(counts) == (1, 1 if accept else 0, 0 if accept else 1)
    assert c.core.lbfgsx_bfgs_ncorr(c.h) == min(npairs + (1 if accept else 0), m)
    c.close()
    ref = oracle.apply_Hv(dtype, m, hist_S, hist_Y, g, -1.0)
    scale = np.abs(ref).max() + 1e-300
    assert np.abs(got - ref).max() <= 4 * np.finfo(dt).eps * scale
    # held to the exact reference, every element (see test_apply_Hv_matches_oracle).  Three of these inputs (n = 70002 rejected in
    # f64, n = 300002 in both types) have an exact dot within the accumulators' worst-case bound of a rounding boundary: there the
    # contract admits two results, and the product is held to the oracle's -- every element as well
    import twoloop_ref as T
    Sr, Yr, ptr = T.ring_fill([(hist_S[k], hist_Y[k]) for k in range(len(hist_S))], m)
    exact = T.two_loop(Sr, Yr, ptr, m, g, -1.0, None, dt)
    assert np.array_equal(got, ref)
    if not exact.ambiguous:
        assert np.array_equal(got, exact.d) and dg.value == exact.dg
    want = float(np.dot(g.astype(f64), got.astype(f64)))
    assert abs(dg.value - want) <= (1e-12 if dtype == O.F64 else 1e-5) * abs(want)


def test_stored_speculative_direction_is_dropped_when_its_inputs_change(A, oracle):
    """lbfgsx_apply_Hv hands out the direction the fused launch computed only if nothing it was computed from
    has changed.  post_linesearch_spec -> stage_correction_host (the spare column now holds ANOTHER pair) -> commit ->
    apply_Hv must recompute: the product on the history with the staged pair, not the speculated one.  Likewise an upload
    into the gradient after the speculation."""
    dtype, n, m, npairs = O.F64, 6000, 5, 3
    rng = np.random.default_rng(5)
    S = rng.standard_normal((npairs, n))
    Y = S * (1.0 + rng.random((npairs, n))) + 0.05 * rng.standard_normal((npairs, n))
    xp, gp = rng.standard_normal(n), rng.standard_normal(n)
    s_new = rng.standard_normal(n)
    x, g = xp + s_new, gp + 1.5 * s_new + 0.05 * rng.standard_normal(n)
    s2 = rng.standard_normal(n)
    y2 = 2.0 * s2 + 0.05 * rng.standard_normal(n)
    g_other = rng.standard_normal(n)
    for variant in ("restage", "upload"):
        c = Ctx(A, dtype, n, m)
        L = c.L
        for k in range(npairs):
            L.check(c.core.lbfgsx_bfgs_add_correction_host(c.h, S[k].ctypes.data_as(C.c_void_p), Y[k].ctypes.data_as(C.c_void_p)))
        c.up(L.VEC_X, xp)
        c.up(L.VEC_G, gp)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        c.up(L.VEC_XT, x)
        c.up(L.VEC_GT, g)
        L.check(c.core.lbfgsx_ls_end(c.h, 0))
        r = [C.c_double() for _ in range(4)]
        L.check(c.core.lbfgsx_post_linesearch_spec(c.h, -1.0, *[C.byref(v) for v in r]))
        counts = (C.c_int64 * 3)()
        c.core.lbfgsx_spec_counts(c.h, C.byref(counts))
        assert tuple(counts) == (1, 0, 0)       # the speculation ran and its pair was accepted
        if variant == "restage":
            sy, yy = C.c_double(), C.c_double()
            c.core.lbfgsx_bfgs_stage_correction_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                                 C.POINTER(C.c_double)]
            L.check(c.core.lbfgsx_bfgs_stage_correction_host(c.h, s2.ctypes.data_as(C.c_void_p), y2.ctypes.data_as(C.c_void_p),
                                                             C.byref(sy), C.byref(yy)))
            L.check(c.core.lbfgsx_commit_correction(c.h))
            hist_S, hist_Y, v = np.vstack([S, s2[None]]), np.vstack([Y, y2[None]]), g
        else:
            L.check(c.core.lbfgsx_commit_correction(c.h))
            c.up(L.VEC_G, g_other)
            hist_S, hist_Y, v = np.vstack([S, (x - xp)[None]]), np.vstack([Y, (g - gp)[None]]), g_other
        dg = C.c_double()
        L.check(c.core.lbfgsx_apply_Hv(c.h, L.VEC_G, -1.0, C.byref(dg)))
        got = c.down(L.VEC_D)
        c.core.lbfgsx_spec_counts(c.h, C.byref(counts))
        assert counts[1] == 0, "the stale speculative direction was handed out (%s)" % variant
        c.close()
        ref = oracle.apply_Hv(dtype, m, hist_S, hist_Y, v, -1.0)
        assert np.abs(got - ref).max() <= 4 * np.finfo(np.float64).eps * np.abs(ref).max()


def test_persistent_launch_recovers_from_a_timed_out_meeting_point(A, monkeypatch):
    """VERDICT r2 / ADVICE r2: one time-out used to switch the persistent launch off for the life of the context.  The
    failure word is pre-set twice during a solve (lbfgsx_debug_persist_fault: the next persistent launch finds it, does
    nothing, the host redoes the product with the step launches): the trajectory is bit-identical to an undisturbed run,
    the context pauses for 8 products each time and then goes back to the persistent form."""
    import gc
    core, _ = A.load()
    n, m, iters = 200002, 6, 44
    x0 = O.rosen_x0(n, 21, O.F64)
    res = {}
    for mode in ("faulted", "clean"):
        gc.collect()
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
        seen = []

        def hook(k, s=s, mode=mode, seen=seen):
            pc = (C.c_int64 * 4)()
            core.lbfgsx_persist_counts(s.ctx, C.byref(pc))
            seen.append(tuple(int(v) for v in pc))
            if mode == "faulted" and k in (4, 24):
                assert core.lbfgsx_debug_persist_fault(s.ctx) == 0
        s.set_iteration_hook(hook)
        x = x0.copy()
        niter, fx = s.minimize(A.ExtendedRosenbrock(), x)
        pc = (C.c_int64 * 4)()
        core.lbfgsx_persist_counts(s.ctx, C.byref(pc))
        res[mode] = (niter, s.last.nfev, fx, x, tuple(int(v) for v in pc), seen)
        del s
    assert res["faulted"][:3] == res["clean"][:3] and np.array_equal(res["faulted"][3], res["clean"][3])
    launches, timeouts, pause, steps = res["faulted"][4]
    assert timeouts == 2 and pause == 0 and 16 <= steps <= 20, res["faulted"][4]
    assert launches >= iters - 20                      # it went back to the persistent form both times
    assert res["clean"][4][1] == 0 and res["clean"][4][3] == 0
    pauses = [t[2] for t in res["faulted"][5]]
    assert max(pauses) <= 8 and pauses.count(0) >= iters - 22   # never more than the 8-product pause: no escalation after a clean launch


def test_two_live_solvers_on_one_device_both_use_the_persistent_kernel(A, oracle):
    """Round 1 used the one-launch recursion only while its context was the single live one of the process.  The
    requirement is narrower -- at most one PERSISTENT kernel in flight per device -- and is kept by a per-device lock held
    for the launch: two live solvers driven alternately both get it, m > 32 included, and nothing changes in the bits."""
    import ctypes as C
    core, _ = A.load()
    core.lbfgsx_persistent_launches.restype = C.c_int64
    core.lbfgsx_persistent_launches.argtypes = [C.c_void_p]
    n = 120002
    x0 = O.rosen_x0(n, 5, O.F64)
    pars = [dict(m=6, it=16), dict(m=40, it=44)]
    solvers = [A.LBFGSSolver(A.LBFGSParam(m=p["m"], epsilon=0.0, epsilon_rel=0.0, max_iterations=p["it"]),
                             linesearch=A.LS_MORE_THUENTE) for p in pars]
    xs = [x0.copy(), x0.copy()]
    out = [None, None]
    for rnd in range(2):           # both contexts stay alive across both rounds
        for k, s in enumerate(solvers):
            xs[k] = x0.copy()
            out[k] = s.minimize(A.ExtendedRosenbrock(), xs[k])
    for k, s in enumerate(solvers):
        assert int(core.lbfgsx_persistent_launches(s.ctx)) > 0, "solver %d fell back to the step launches" % k
        x_ref, r = oracle.lbfgs(O.F64, O.LS_MT, O.OBJ_ROSEN, x0, O.lbfgs_params(m=pars[k]["m"], epsilon=0, epsilon_rel=0,
                                                                                max_iterations=pars[k]["it"]))
        assert (r.niter, r.nfev) == (out[k][0], s.last.nfev) and np.array_equal(xs[k], x_ref)


@pytest.mark.parametrize("obj,ls,window,tol", [(O.OBJ_ROSEN, O.LS_MT, 40, 1e-10), (O.OBJ_QUAD, O.LS_NW, 50, 1e-12)])
def test_drift_against_the_native_accumulator_reference(A, obj, ls, window, tol):
    """north_star: "match the Eigen reference iterate-for-iterate within 1e-10".  Every other trajectory test compares
    with the reference built on extended-precision sums (bit-identical); this one compares with the SAME reference
    headers built with native accumulators (plain f64 sums in index order: Eigen's reductions up to their packet order,
    oracle/_ref/libref_native.so).  A different summation order alone separates two correct runs chaotically (SURVEY
    7(1e)), so the bound holds over a window: 1e-10 through the first 40 objective evaluations (about 30 iterations)
    of the extended Rosenbrock run -- the full curve, which leaves the band at evaluation ~50, is committed as
    profiles/r2_drift_native_accumulators.json (scripts/drift_curves.py native) -- and 1e-12 over all 40 iterations of
    the convex quadratic.  Reference: BFGSMat.h:276-302, LBFGS.h:78-173."""
    if not O.available("ref", "native"):
        pytest.skip("oracle/_ref/libref_native.so not built")
    nat = O.Oracle("ref", "native")
    n, m, iters = 200000, 10, 40
    p = O.lbfgs_params(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters)
    if obj == O.OBJ_ROSEN:
        x0, a, b, f = O.rosen_x0(n), None, None, A.ExtendedRosenbrock()
    else:
        a, b = O.quad_problem(n, 10.0, 1, O.F64)
        x0, f = np.zeros(n), A.DiagQuadratic(a, b)
    tn, tg = O.TraceBuf(n, cap=512, stride=7), A.TraceBuffer(n, cap=512, stride=7)
    xn, rn = nat.lbfgs(O.F64, ls, obj, x0, p, a=a, b=b, trace=tn)
    s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters),
                      linesearch=A.LS_MORE_THUENTE if ls == O.LS_MT else A.LS_NOCEDAL_WRIGHT)
    x = x0.copy()
    niter, fx = s.minimize(f, x, trace=tg)
    assert (niter, s.last.nfev) == (rn.niter, rn.nfev)    # same decisions all the way
    k = min(window, tg.count)
    err = np.abs(tg.xs[:k] - tn.xs[:k]).max(axis=1)
    assert err.max() <= tol, "evaluation %d deviates by %.3g" % (int(err.argmax()), err.max())
    assert err[:8].max() <= 1e-13                          # SURVEY probe: 1.7e-13 at K = 10


def test_fused_persistent_launch_signals_a_polling_host_and_changes_no_bit(A, monkeypatch):
    """Round 6: with host-mapped outputs the fused persistent launch's closing block stores the six scalars the host reads next
    with system-scope stores and then the completion word; the host polls (no copies, no stream wait) while the blocks still
    store the resident part of d.  Against LBFGSX_PERSIST_POLL=0 (copies + stream wait) and LBFGSX_MAPPED_OUT=0 (round 5's
    L-BFGS path): the same trajectory bit for bit; the waits are served by polling and none runs into the time-out."""
    import ctypes as C
    from lbfgspp_amd import _lib as L
    core, _ = L.load()
    n, iters = 6_000_000, 30
    res = {}
    for name, mapped, ppoll in (("poll", "1", "1"), ("copies", "1", "0"), ("round5", "0", "0")):
        monkeypatch.setenv("LBFGSX_MAPPED_OUT", mapped)
        monkeypatch.setenv("LBFGSX_PERSIST_POLL", ppoll)
        s = A.LBFGSSolver(A.LBFGSParam(m=7, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
        ctx = s.prepare(n)
        L.check(core.lbfgsx_gen_rosen_x0(ctx, 7))
        niter, fx = s.minimize_resident(A.ExtendedRosenbrock(), n)
        x = np.empty(n)
        L.check(core.lbfgsx_download(ctx, L.VEC_X, x.ctypes.data_as(C.c_void_p)))
        pc = (C.c_int64 * 4)()
        L.check(core.lbfgsx_poll_counts_ex(ctx, C.byref(pc)))
        res[name] = (niter, s.last.nfev, fx, x, [int(v) for v in pc])
        s.close()
    for other in ("copies", "round5"):
        assert res["poll"][:3] == res[other][:3] and np.array_equal(res["poll"][3], res[other][3]), other
    waits, timeouts, bad, off = res["poll"][4]
    assert waits >= 2 * iters - 4 and timeouts == 0 and bad == 0 and off == 0   # every trial and every fused launch
    assert res["round5"][4][0] == 0
    assert res["copies"][4][0] < waits
