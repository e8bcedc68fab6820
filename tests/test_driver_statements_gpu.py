"""-m gpu: the driver-statement kernels, each called directly through the C ABI and compared with the references of
tests/statement_ref.py (proved on the CPU by tests/test_statement_ref_cpu.py):

  * vectors (x, g, s, y, d) bit for bit against numpy in the same dtype, one numpy operation per operation of the kernel;
  * sums (f, g.g, x.x, g.d, s.y, y.y) adjacent to the exact sum of the T-rounded terms: one of the two T values that
    bracket it (statement_ref.adjacent; every input is checked to satisfy sum|t| <= 2^20 |sum t| first);
  * extrema (projected-gradient norm, step_max) exactly equal.

Objectives: the two built-in ones and two term bodies compiled at run time (CHAIN2: K = 2, data that depends on the index;
ALLSLOTS: K = 1, all four data slots and all eight scalars).  Shapes: statement_ref.edge_sizes (around the pack width, the
block, the tile of the trial kernels, the capped grid, ~3e6).  Finite inputs only, apart from infinite bounds."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
import statement_ref as R

pytestmark = pytest.mark.gpu

NPDT = {O.F64: np.float64, O.F32: np.float32}
OBJS = {"quad": 1, "rosen": 2, "chain2": 2, "allslots": 1}  # name -> K
STEPS = [1.0, 0.37, 0.1, 2.0 ** -30]  # 0.37 and 0.1 are not representable in float (nor double): the library converts with T(step)
SMALL = 20000  # up to here a test walks every bound edge; above it a selection (time on the host, not on the device)


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


def _sizes(dtype, K=1, big=True):
    """big = False: without the ~3e6 case (host time of the exact sums); the capped-grid case stays"""
    out = []
    for n in R.edge_sizes(NPDT[dtype], True):
        if n >= 3_000_000 and not big:
            continue
        n = R.nearest_even(n) if K == 2 else n
        if n not in out:
            out.append(n)
    return out


def _params(objs=("quad", "rosen", "chain2", "allslots"), big=True):
    ps = []
    for dtype in (O.F64, O.F32):
        for obj in objs:
            for n in _sizes(dtype, OBJS[obj] if obj else 1, big):
                ps.append(pytest.param(dtype, obj, n, id="%s-%s-%d" % ("f64" if dtype == O.F64 else "f32", obj, n)))
    return ps


def _params_plain(big=True):
    return [pytest.param(dtype, n, id="%s-%d" % ("f64" if dtype == O.F64 else "f32", n)) for dtype in (O.F64, O.F32)
            for n in _sizes(dtype, 1, big)]


_compiled = {}  # (body name, dtype) -> handle; a compiled body stays for the process anyway


def _d(k):
    return [C.c_double(math.nan) for _ in range(k)]


class Ctx:
    def __init__(self, A, dtype, n, bounded=False, m=3):
        from lbfgspp_amd import _lib as L
        self.L = L
        self.core, _ = A.load()
        self.h = C.c_void_p()
        self.dtype, self.n, self.dt, self.m = dtype, n, NPDT[dtype], m
        L.check(self.core.lbfgsx_create(C.byref(self.h), dtype, n, m, 0, L.FLAG_BOUNDED if bounded else 0))

    def up(self, which, arr):
        arr = np.ascontiguousarray(arr, self.dt)
        assert arr.size == self.n
        self.L.check(self.core.lbfgsx_upload(self.h, which, arr.ctypes.data_as(C.c_void_p)))

    def down(self, which):
        out = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self.h:
            self.core.lbfgsx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def objective(self, name, rng):
        """binds / uploads the objective's data; returns (objective id for the ABI, x -> (g, terms, factor))"""
        L, n, dt = self.L, self.n, self.dt
        if name == "rosen":
            return L.OBJ_EXT_ROSENBROCK, R.rosen_ref
        if name == "quad":
            a, b = (0.5 + rng.random(n)).astype(dt), rng.standard_normal(n).astype(dt)
            self.up(L.VEC_A, a)
            self.up(L.VEC_B, b)
            return L.OBJ_DIAG_QUAD, lambda x: R.quad_ref(x, a, b)
        body = {"chain2": R.CHAIN2, "allslots": R.ALLSLOTS}[name]
        key = (name, self.dtype)
        if key not in _compiled:
            h = C.c_void_p()
            log = C.create_string_buffer(8192)
            rc = self.core.lbfgsx_objective_compile(C.byref(h), self.dtype, OBJS[name], body.encode(), log, len(log))
            assert rc == 0 and h.value, log.value.decode()
            _compiled[key] = h
        data = R.term_data(rng, n, dt)
        nslots = 2 if name == "chain2" else 4
        ptrs = (C.c_void_p * 4)()
        for slot in range(nslots):
            dev = C.c_void_p()
            L.check(self.core.lbfgsx_objective_upload(self.h, slot, data[slot].ctypes.data_as(C.c_void_p), C.byref(dev)))
            assert dev.value
            ptrs[slot] = dev.value
        cs = (C.c_double * 8)(*(R.ALLSLOTS_SCALARS if name == "allslots" else [0.0] * 8))
        oid = C.c_int(-1)
        L.check(self.core.lbfgsx_objective_bind(self.h, _compiled[key], C.byref(ptrs), C.byref(cs), C.byref(oid)))
        assert oid.value == L.OBJ_BOUND
        if name == "chain2":
            return oid.value, lambda x: R.chain2_ref(x, data[0], data[1])
        return oid.value, lambda x: R.allslots_ref(x, *data)


def _sum_ok(got, terms, dt, what, scale=1):
    ok, msg = R.check_sum(got, np.asarray(terms, np.float64), dt, scale)
    print("%s: %s" % (what, msg))
    assert ok, "%s is not adjacent to the exact sum: %s" % (what, msg)


def _dot_ok(got, a, b, dt, what):
    _sum_ok(got, R.dot_terms(a, b), dt, what)


def _bits(got, want, what):
    assert got.dtype == want.dtype
    same = got.view(np.uint8).reshape(got.size, -1) == want.view(np.uint8).reshape(want.size, -1)
    if not same.all():
        bad = np.flatnonzero(~same.all(axis=1))
        raise AssertionError("%s differs from the reference in %d of %d elements, first at %d: got %r, want %r"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def _launches(core):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), 0) == 0
    return cnt[0]


def _ahead(c):
    out = (C.c_int64 * 2)()
    assert c.core.lbfgsx_b_trial_ahead_counts(c.h, C.byref(out)) == 0
    return out[0], out[1]


def _bound_cases(rng, n, dt):
    cases = R.bound_cases(rng, n, dt)
    if n > SMALL:
        cases = {k: cases[k] for k in ("mixed_one_sided", "limit_tail", "on_bound_outward_lower")}
    return cases


# ---------------------------------------------------------------- lbfgsx_eval, lbfgsx_b_eval
@pytest.mark.parametrize("dtype,obj,n", _params())
def test_eval_statement(A, dtype, obj, n):
    """k_eval: g bit-equal, f, g.g and x.x adjacent to the exact sums"""
    rng = np.random.default_rng(1000 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = c.objective(obj, rng)
        x = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, x)
        fx, g2, x2 = _d(3)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        g = c.down(L.VEC_G)
    g_ref, terms, scale = ref(x)
    _bits(g, g_ref, "g")
    _sum_ok(fx.value, terms, dt, "f", scale)
    _dot_ok(g2.value, g_ref, g_ref, dt, "g.g")
    _dot_ok(x2.value, x, x, dt, "x.x")


@pytest.mark.parametrize("dtype,obj,n", _params())
def test_b_eval_statement(A, dtype, obj, n):
    """k_b_eval: g bit-equal, f and x.x adjacent, the projected-gradient norm exactly equal -- on every bound edge"""
    rng = np.random.default_rng(2000 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = c.objective(obj, rng)
        for name, (x, _, lb, ub) in _bound_cases(rng, n, dt).items():
            c.up(L.VEC_X, x)
            c.up(L.VEC_LB, lb)
            c.up(L.VEC_UB, ub)
            fx, pg, x2 = _d(3)
            L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
            g = c.down(L.VEC_G)
            g_ref, terms, scale = ref(x)
            _bits(g, g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f", scale)
            _dot_ok(x2.value, x, x, dt, name + ": x.x")
            assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), name + ": projected-gradient norm"


# ---------------------------------------------------------------- lbfgsx_ls_begin + lbfgsx_trial
def _trial_ref(ref, xp, d, step):
    xt = R.axpy_ref(xp, d, step)
    g_ref, terms, scale = ref(xt)
    return xt, g_ref, terms, scale


def _check_trial(c, ref, xp, d, step, fx, dg, what):
    L, dt = c.L, c.dt
    xt_ref, g_ref, terms, scale = _trial_ref(ref, xp, d, step)
    xt, gt = c.down(L.VEC_XT), c.down(L.VEC_GT)
    _bits(xt, xt_ref, what + ": x trial")
    _bits(gt, g_ref, what + ": g trial")
    _sum_ok(fx, terms, dt, what + ": f", scale)
    _dot_ok(dg, g_ref, d, dt, what + ": g.d")
    return xt, gt


@pytest.mark.parametrize("dtype,obj,n", _params())
def test_trial_statement_in_both_tile_orders(A, dtype, obj, n):
    """k_trial twice at the same step: the tile order alternates per launch, both orders give the reference's bits"""
    rng = np.random.default_rng(3000 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = c.objective(obj, rng)
        xp = rng.standard_normal(n).astype(dt)
        d = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, xp)
        c.up(L.VEC_D, d)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        _bits(c.down(L.VEC_XP), xp, "xp after ls_begin")
        stale = np.full(n, -77.0, dt)
        for step in (STEPS if n <= SMALL else STEPS[1:2]):
            runs = []
            for k in range(2):
                c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible
                c.up(L.VEC_GT, stale)
                fx, dg = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                assert _launches(c.core) == before + 1
                if k == 0:  # the second launch is compared with the first, bit for bit, below
                    xt, gt = _check_trial(c, ref, xp, d, step, fx.value, dg.value, "step %r" % step)
                else:
                    xt, gt = c.down(L.VEC_XT), c.down(L.VEC_GT)
                runs.append((fx.value, dg.value, xt, gt))
            assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], "f or g.d depends on the tile order"
            _bits(runs[0][2], runs[1][2], "x trial of the two tile orders")
            _bits(runs[0][3], runs[1][3], "g trial of the two tile orders")


@pytest.mark.parametrize("dtype,n", _params_plain())
def test_trial_point_trial_dg_and_norms(A, dtype, n):
    """the device-functor path: k_axpy_point, then k_dot on a gradient the caller wrote; lbfgsx_norms on (g, x)"""
    rng = np.random.default_rng(4000 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        xp, d, gt, g = (rng.standard_normal(n).astype(dt) for _ in range(4))
        c.up(L.VEC_X, xp)
        c.up(L.VEC_G, g)
        c.up(L.VEC_D, d)
        g2, x2 = _d(2)
        L.check(c.core.lbfgsx_norms(c.h, C.byref(g2), C.byref(x2)))
        _dot_ok(g2.value, g, g, dt, "g.g")
        _dot_ok(x2.value, xp, xp, dt, "x.x")
        L.check(c.core.lbfgsx_ls_begin(c.h))
        for step in STEPS:
            L.check(c.core.lbfgsx_trial_point(c.h, step))
            _bits(c.down(L.VEC_XT), R.axpy_ref(xp, d, step), "x trial, step %r" % step)
        c.up(L.VEC_GT, gt)
        dg = C.c_double(math.nan)
        L.check(c.core.lbfgsx_trial_dg(c.h, C.byref(dg)))
        _dot_ok(dg.value, gt, d, dt, "g.d")
        _bits(c.down(L.VEC_XP), xp, "xp")
        _bits(c.down(L.VEC_D), d, "d")


# ---------------------------------------------------------------- lbfgsx_post_linesearch, lbfgsx_b_post_linesearch
def _history(c):
    S, Y = np.empty(c.n, c.dt), np.empty(c.n, c.dt)
    ncorr, ptr, theta = C.c_int(-1), C.c_int(-1), C.c_double(math.nan)
    c.L.check(c.core.lbfgsx_bfgs_download_history(c.h, S.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), C.byref(ncorr),
                                                  C.byref(ptr), C.byref(theta)))
    assert ncorr.value == 1
    return S, Y, theta.value


def _accepted_point(c, rng):
    """xp, gp at the start of a search and an accepted trial point x, g with s.y > 0, placed in the context's buffers"""
    L, n, dt = c.L, c.n, c.dt
    xp, gp = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    s0 = rng.standard_normal(n)
    x = (xp + 0.3 * s0).astype(dt)
    g = (gp + 0.3 * s0 * (1.0 + rng.random(n)) + 0.02 * rng.standard_normal(n)).astype(dt)
    c.up(L.VEC_X, xp)
    c.up(L.VEC_G, gp)
    L.check(c.core.lbfgsx_ls_begin(c.h))
    c.up(L.VEC_XT, x)
    c.up(L.VEC_GT, g)
    L.check(c.core.lbfgsx_ls_end(c.h, 0))
    return xp, gp, x, g


@pytest.mark.parametrize("dtype,n", _params_plain(big=False))
def test_post_linesearch_statement(A, dtype, n):
    """k_post twice (both tile orders): s and y bit-equal in the history after the commit, the four sums adjacent"""
    rng = np.random.default_rng(5000 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        xp, gp, x, g = _accepted_point(c, rng)
        s_ref, y_ref = R.sy_ref(x, xp, g, gp)
        runs = []
        for k in range(2):
            r = _d(4)
            L.check(c.core.lbfgsx_post_linesearch(c.h, *[C.byref(v) for v in r]))
            runs.append([v.value for v in r])
        assert runs[0] == runs[1], "a sum depends on the tile order"
        g2, x2, sy, yy = runs[0]
        L.check(c.core.lbfgsx_commit_correction(c.h))
        S, Y, theta = _history(c)
    _bits(S, s_ref, "s")
    _bits(Y, y_ref, "y")
    _dot_ok(g2, g, g, dt, "g.g")
    _dot_ok(x2, x, x, dt, "x.x")
    _dot_ok(sy, s_ref, y_ref, dt, "s.y")
    _dot_ok(yy, y_ref, y_ref, dt, "y.y")
    assert theta == float(dt(dt(yy) / dt(sy))), "theta = y.y / s.y in T (BFGSMat.h:92)"


@pytest.mark.parametrize("dtype,n", _params_plain(big=False))
def test_b_post_linesearch_statement(A, dtype, n):
    rng = np.random.default_rng(6000 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        xp, gp, x, g = _accepted_point(c, rng)
        s_ref, y_ref = R.sy_ref(x, xp, g, gp)
        out = {}
        for name, (_, _, lb, ub) in _bound_cases(rng, n, dt).items():
            # bounds around another point: x lies inside some, outside others -- the statement takes any x
            c.up(L.VEC_LB, lb)
            c.up(L.VEC_UB, ub)
            r = _d(4)
            L.check(c.core.lbfgsx_b_post_linesearch(c.h, *[C.byref(v) for v in r]))
            pg, x2, sy, yy = [v.value for v in r]
            assert pg == R.projg_norm_ref(x, g, lb, ub), name + ": projected-gradient norm"
            out[name] = (x2, sy, yy)
        assert len(set(out.values())) == 1, "the sums depend on the bounds"
        L.check(c.core.lbfgsx_commit_correction(c.h))
        S, Y, theta = _history(c)
    _bits(S, s_ref, "s")
    _bits(Y, y_ref, "y")
    _dot_ok(x2, x, x, dt, "x.x")
    _dot_ok(sy, s_ref, y_ref, dt, "s.y")
    _dot_ok(yy, y_ref, y_ref, dt, "y.y")
    assert theta == float(dt(dt(yy) / dt(sy)))


# ---------------------------------------------------------------- lbfgsx_b_dg_maxstep, lbfgsx_b_dg_maxstep_trial
def _step_max_ok(got, x, d, lb, ub, name):
    want = R.step_max_ref(x, d, lb, ub)
    assert got == want, "%s: step_max %r, reference %r" % (name, got, want)
    if name in ("all_infinite", "d_zero"):
        assert got == math.inf
    if name.startswith("on_bound_outward"):
        assert got == 0.0 and math.copysign(1.0, got) == 1.0, name + ": the quotient -0 must come out as +0"


@pytest.mark.parametrize("ahead", [None, "0"], ids=["trial_ahead", "trial_ahead_off"])
@pytest.mark.parametrize("dtype,obj,n", _params(big=False))
def test_dg_maxstep_and_its_fused_first_trial(A, monkeypatch, dtype, obj, n, ahead):
    """k_b_dg_maxstep and k_b_dg_maxstep_trial on every bound edge: g.d adjacent, step_max exact; the fused form also leaves the
    trial point, its gradient, f and grad.d of lbfgsx_trial, which hands them out without a launch for exactly that step and
    recomputes for another.  With LBFGSX_TRIAL_AHEAD=0 the same calls give the same values from separate launches."""
    if ahead is None:
        monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    else:
        monkeypatch.setenv("LBFGSX_TRIAL_AHEAD", ahead)
    rng = np.random.default_rng(7000 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = c.objective(obj, rng)
        for name, (x, d, lb, ub) in _bound_cases(rng, n, dt).items():
            g0 = rng.standard_normal(n).astype(dt)
            for which, arr in ((L.VEC_X, x), (L.VEC_G, g0), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                c.up(which, arr)
            L.check(c.core.lbfgsx_ls_begin(c.h))
            dg, sm = _d(2)
            L.check(c.core.lbfgsx_b_dg_maxstep(c.h, C.byref(dg), C.byref(sm)))
            _dot_ok(dg.value, g0, d, dt, name + ": g.d")
            _step_max_ok(sm.value, x, d, lb, ub, name)
            # the fused form at step0, then the search's first trial at exactly step0, then a trial elsewhere
            step0, step1 = (0.37, 0.1) if name != "limit_first" else (1.0, 2.0 ** -30)
            runs0, hits0 = _ahead(c)
            dg2, sm2 = _d(2)
            L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg2), C.byref(sm2)))
            assert (dg2.value, sm2.value) == (dg.value, sm.value), name + ": the two kernels disagree"
            _step_max_ok(sm2.value, x, d, lb, ub, name + " (fused)")
            runs1, hits1 = _ahead(c)
            fused = runs1 == runs0 + 1
            assert fused == (ahead is None), "trial evaluated ahead: %s, LBFGSX_TRIAL_AHEAD=%r" % (fused, ahead)
            if fused:  # what the pass left in the trial buffers, before lbfgsx_trial is asked
                _bits(c.down(L.VEC_XT), R.axpy_ref(x, d, step0), name + ": x trial left by the fused pass")
                _bits(c.down(L.VEC_GT), ref(R.axpy_ref(x, d, step0))[0], name + ": g trial left by the fused pass")
            fx, dgt = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
            assert _launches(c.core) == before + (0 if fused else 1), "the kept trial must be handed out without a launch"
            assert _ahead(c) == (runs1, hits1 + (1 if fused else 0))
            _check_trial(c, ref, x, d, step0, fx.value, dgt.value, name + ": first trial at step0")
            fx, dgt = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step1, C.byref(fx), C.byref(dgt)))
            assert _launches(c.core) == before + 1 and _ahead(c) == (runs1, hits1 + (1 if fused else 0))
            _check_trial(c, ref, x, d, step1, fx.value, dgt.value, name + ": trial at another step")
            _bits(c.down(L.VEC_G), g0, name + ": g at xp is left alone")


# ---------------------------------------------------------------- lbfgsx_b_force_bounds, lbfgsx_b_dir_from_xcp, lbfgsx_b_dot_drt_g, lbfgsx_b_norms
@pytest.mark.parametrize("dtype,n", _params_plain(big=False))
def test_force_bounds_direction_from_xcp_and_norms(A, dtype, n):
    rng = np.random.default_rng(8000 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        for name, (x, _, lb, ub) in _bound_cases(rng, n, dt).items():
            g = rng.standard_normal(n).astype(dt)
            xo = (x + 2.0 * rng.standard_normal(n)).astype(dt)  # outside the bounds on many coordinates
            c.up(L.VEC_LB, lb)
            c.up(L.VEC_UB, ub)
            c.up(L.VEC_X, xo)
            c.up(L.VEC_G, g)
            pg, x2 = _d(2)
            L.check(c.core.lbfgsx_b_norms(c.h, C.byref(pg), C.byref(x2)))  # takes any x
            assert pg.value == R.projg_norm_ref(xo, g, lb, ub), name + ": projected-gradient norm"
            _dot_ok(x2.value, xo, xo, dt, name + ": x.x")
            L.check(c.core.lbfgsx_b_force_bounds(c.h))
            xc = c.down(L.VEC_X)
            _bits(xc, R.clamp_ref(xo, lb, ub), name + ": clamped x")
            assert np.all(xc >= lb) and np.all(xc <= ub)
            # d = xcp - x, plain and normalised
            xcp = R.clamp_ref((xc - 0.5 * g).astype(dt), lb, ub)
            c.up(L.VEC_XCP, xcp)
            d_ref = R.dir_from_xcp_ref(xcp, xc)
            L.check(c.core.lbfgsx_b_dir_from_xcp(c.h, 0))
            _bits(c.down(L.VEC_D), d_ref, name + ": d = xcp - x")
            dg = C.c_double(math.nan)
            L.check(c.core.lbfgsx_b_dot_drt_g(c.h, C.byref(dg)))
            _dot_ok(dg.value, d_ref, g, dt, name + ": d.g")
            L.check(c.core.lbfgsx_b_dir_from_xcp(c.h, 1))
            dn = c.down(L.VEC_D)
            cands = R.normalized_candidates(d_ref)
            assert any(np.array_equal(dn, cand) for cand in cands), \
                name + ": normalised d equals d / T(sqrt(z)) for neither T value z adjacent to the exact d.d"
            _bits(c.down(L.VEC_X), xc, name + ": x is left alone")
        # xcp == x: d = 0, the squared norm is not positive, nothing is divided
        c.up(L.VEC_XCP, xc)
        L.check(c.core.lbfgsx_b_dir_from_xcp(c.h, 1))
        _bits(c.down(L.VEC_D), np.zeros(n, dt), "d = 0")
        dg = C.c_double(math.nan)
        L.check(c.core.lbfgsx_b_dot_drt_g(c.h, C.byref(dg)))
        assert dg.value == 0.0
