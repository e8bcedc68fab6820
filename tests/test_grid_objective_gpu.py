"""-m gpu: grid objectives (lbfgspp_amd.GridObjective, csrc/grid_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/grid_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * a grid objective whose cells ignore the row below equals the K = 2 chain objective of the same row-wise body;
  * the Allen-Cahn energy follows the reference (tests/golden/grid_golden.json), from Python and from C++;
  * a 64 x 64 Allen-Cahn problem converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import grid_ref as GR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates of a 16-byte pack
TRIAL_U = 2                  # grid_kernels.cuh: kGridTrialU, the tile depth of the two trial kernels
# the capped grid is 1024 blocks and a tile of the trial kernels 512 packs: from 2 * 1024 tiles on every block walks its stride
# twice (the evaluation kernels, whose step is a block's 256 packs, four times); cols even: the aligned path
WRAP_F64 = (1025, 2052)
# f32: a tile of the trial kernels is 2048 coordinates, so 2052 tiles again; and one column more: the unaligned path, where the
# position carried from tile to tile is advanced and retreated by a step with a column part
WRAP_F32 = ((1025, 4100), (1025, 4101))


def _shape_list(dtype):
    W = PACK[dtype]
    shapes = [(2, 2), (2, 3), (3, 2), (3, 5), (5, 3)]
    # cols around the pack: the unaligned path, rows that straddle packs (cols = W - 1 = 1 is no grid in f64)
    shapes += [(rows, cols) for cols in (W - 1, W, W + 1, 2 * W + 1) if cols >= 2 for rows in (3, 4)]
    shapes += [(3, cols) for cols in (64 * W - W, 64 * W, 64 * W + W, 64 * W + 1)]        # a wave's span
    shapes += [(3, cols) for cols in (256 * W - W, 256 * W + W, 256 * W + 1)]             # a block's span
    shapes += [(3, cols) for cols in (TRIAL_U * 256 * W - W, TRIAL_U * 256 * W + W)]      # a trial tile's span
    shapes += [(4099, 2), (4099, 3), (3, 43)]                                              # tall and thin; a flat tail
    shapes += [WRAP_F64] if dtype == O.F64 else list(WRAP_F32)
    return shapes


def _shapes():
    return [pytest.param(dtype, rows, cols, id="%s-%dx%d" % ("f64" if dtype == O.F64 else "f32", rows, cols))
            for dtype in (O.F64, O.F32) for rows, cols in dict.fromkeys(_shape_list(dtype))]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, body):
    key = (body, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_grid(C.byref(h), c.dtype, body.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _bind(c, rows, cols, rng):
    """compiles (once per process) and binds ASYM4 with random per-node weights; returns (id, x -> (g, cell values))"""
    L, n, dt = c.L, c.n, c.dt
    assert n == rows * cols
    p0 = (0.5 + rng.random(n)).astype(dt)
    ptrs = (C.c_void_p * 4)()
    dev = C.c_void_p()
    L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(*(GR.ASYM_SCALARS + (0.0,) * 6))
    oid = C.c_int(-1)
    L.check(c.core.lbfgsx_objective_bind_grid(c.h, _compile(c, GR.ASYM4), rows, cols, C.byref(ptrs), C.byref(cs), C.byref(oid)))
    assert oid.value == L.OBJ_BOUND
    r, cc = C.c_int64(0), C.c_int64(0)
    assert c.core.lbfgsx_objective_shape(c.h, C.byref(r), C.byref(cc)) == 0 and (r.value, cc.value) == (rows, cols)

    def ref(x):
        tg, v = GR.asym4_terms(x, rows, cols, p0)
        return GR.grid_grad(tg, rows, cols), v.reshape(-1)
    return oid.value, ref


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,rows,cols", _shapes())
def test_eval_statement(A, dtype, rows, cols):
    n = rows * cols
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, rows, cols, rng)
        x = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, x)
        fx, g2, x2 = _d(3)
        before = _launches(c.core)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        assert _launches(c.core) == before + 1
        g = c.down(L.VEC_G)
    g_ref, terms = ref(x)
    _bits(g, g_ref, "g")
    _sum_ok(fx.value, terms, dt, "f")
    _dot_ok(g2.value, g_ref, g_ref, dt, "g.g")
    _dot_ok(x2.value, x, x, dt, "x.x")


@pytest.mark.parametrize("dtype,rows,cols", _shapes())
def test_trial_statement_in_both_tile_orders(A, dtype, rows, cols):
    n = rows * cols
    rng = np.random.default_rng(200 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, rows, cols, rng)
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


@pytest.mark.parametrize("dtype,rows,cols", _shapes())
def test_b_eval_statement(A, dtype, rows, cols):
    n = rows * cols
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, rows, cols, rng)
        cases = R.bound_cases(rng, n, dt)
        for name in cases if n <= 20000 else ["mixed_one_sided"]:
            x, _, lb, ub = cases[name]
            c.up(L.VEC_X, x)
            c.up(L.VEC_LB, lb)
            c.up(L.VEC_UB, ub)
            fx, pg, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g = c.down(L.VEC_G)
            g_ref, terms = ref(x)
            _bits(g, g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(x2.value, x, x, dt, name + ": x.x")
            assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), name


@pytest.mark.parametrize("dtype,rows,cols", _shapes())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, rows, cols):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    n = rows * cols
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, rows, cols, rng)
        cases = R.bound_cases(rng, n, dt)
        for name in cases if n <= 20000 else ["mixed_one_sided"]:
            x, d, lb, ub = cases[name]
            g0 = rng.standard_normal(n).astype(dt)
            for which, arr in ((L.VEC_X, x), (L.VEC_G, g0), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                c.up(which, arr)
            L.check(c.core.lbfgsx_ls_begin(c.h))
            step0 = 0.37
            runs0, hits0 = _ahead(c)
            dg, sm = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
            assert _launches(c.core) == before + 1
            assert _ahead(c) == (runs0 + 1, hits0), "the fused kernel did not run"
            xt_ref = R.axpy_ref(x, d, step0)
            g_ref, terms = ref(xt_ref)
            _bits(c.down(L.VEC_XT), xt_ref, name + ": x trial left by the fused pass")
            _bits(c.down(L.VEC_GT), g_ref, name + ": g trial left by the fused pass")
            fx, dgt = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
            assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)
            _bits(c.down(L.VEC_G), g0, name + ": g at xp is left alone")
            _dot_ok(dg.value, g0, d, dt, name + ": g.d")
            assert sm.value == R.step_max_ref(x, d, lb, ub), name
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(dgt.value, g_ref, d, dt, name + ": grad(x).d")


# ---------------------------------------------------------------- a grid that ignores the row below is a chain
@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("rows,cols", [(5, 131), (37, 40)])
def test_row_wise_grid_is_the_chain_of_the_same_body(A, dtype, rows, cols):
    """the extended Rosenbrock function cannot be restated as a grid (its pairs are not cells); instead a cell body that
    ignores x[2] and x[3] is the K = 2 chain of the same row-wise body, with a weight p0 that is zero where the chain would
    cross a row end and on the last row (no cell starts there).  The gradients are compared with == on values: the grid's
    dead partials enter its sums as +0, the chain's cut terms as +-0, so a zero's sign may differ and nothing else."""
    n = rows * cols
    rng = np.random.default_rng(n)
    dt = NPDT[dtype]
    p0 = (0.5 + rng.random(n)).astype(dt).reshape(rows, cols)
    p0[:, -1] = 0
    p0[-1, :] = 0
    p0 = p0.reshape(-1)
    x = rng.standard_normal(n).astype(dt)
    got = {}
    with Ctx(A, dtype, n) as c:
        L = c.L
        ptrs = (C.c_void_p * 4)()
        dev = C.c_void_p()
        L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
        ptrs[0] = dev.value
        c.up(L.VEC_X, x)
        hc = C.c_void_p()
        log = C.create_string_buffer(8192)
        assert c.core.lbfgsx_objective_compile_chain(C.byref(hc), dtype, 2, GR.ROW_PAIR_CHAIN.encode(), log, len(log)) == 0, log.value
        oid = C.c_int(-1)
        for name in ("chain", "grid"):
            if name == "chain":
                L.check(c.core.lbfgsx_objective_bind(c.h, hc, C.byref(ptrs), None, C.byref(oid)))
            else:
                L.check(c.core.lbfgsx_objective_bind_grid(c.h, _compile(c, GR.ROW_PAIR_GRID), rows, cols, C.byref(ptrs), None,
                                                          C.byref(oid)))
            fx, g2, x2 = _d(3)
            L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
            got[name] = (c.down(L.VEC_G).copy(), fx.value)
        c.core.lbfgsx_objective_destroy(hc)
    assert np.array_equal(got["chain"][0], got["grid"][0])
    assert np.any(got["grid"][0] != 0) and np.all(got["grid"][0].reshape(rows, cols)[-1] == 0)
    # the same terms, summed by the order-independent sum of both forms
    assert got["chain"][1] == got["grid"][1]


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "grid_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(rows, cols):
    """tests/cpp/grid_probe.cpp: start() -- a smooth bump scaled into the box [-0.5, 2], operation for operation"""
    tr = (np.arange(rows, dtype=np.float64)[:, None] + 1.0) / float(rows + 1)
    tc = (np.arange(cols, dtype=np.float64)[None, :] + 1.0) / float(cols + 1)
    bump = (tr * (1.0 - tr)) * (tc * (1.0 - tc))
    return (-0.3 + (16.0 * bump) * ((1.0 + 0.5 * tr) + 0.25 * tc)).reshape(-1)


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%dx%d" % (i["solver"], i["rows"], i["cols"]))
def test_allen_cahn_follows_the_reference(A, inst):
    rows, cols, tol = inst["rows"], inst["cols"], 1e-10
    n = rows * cols
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(rows, cols)
        f = A.GridObjective(GR.ALLENCAHN, shape=(rows, cols), scalars=(c0,))
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


def test_cpp_grid_objective_follows_the_reference(tmp_path):
    """tests/cpp/grid_probe.cpp with GridObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "grid_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DGRID_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "grid_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["rows"], i["cols"]) for i in insts}):
        mine = [i for i in insts if (i["rows"], i["cols"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe, str(shape[0]), str(shape[1]), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert out.returncode == 0 and "GRID PROBE OK" in out.stdout, out.stdout[-2000:]
        rows_ = {}
        for line in out.stdout.splitlines():
            w = line.split()
            if w and w[0] in ("lbfgs", "lbfgsb"):
                rows_[(w[0], int(w[1]))] = (int(w[2]), float(w[4]), np.array([float(v) for v in w[5:]]))
        for inst in mine:
            for k in range(1, inst["iterations"] + 1):
                niter, fx, x = rows_[(inst["solver"], k)]
                x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
                assert niter == inst["niter"][k - 1]
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], shape, k)


# ---------------------------------------------------------------- convergence
def _allencahn_grad(x, rows, cols, c0):
    """the gradient in double, written independently of the body: the half-weighted edge Laplacian plus the potential's
    derivative c0 (x^2 - 1) x on the nodes a cell starts at"""
    X = x.reshape(rows, cols)
    g = np.zeros((rows, cols))
    wh = np.full((rows, cols - 1), 1.0)   # horizontal edges: in two cells unless on the first or last row
    wh[0] = wh[-1] = 0.5
    wv = np.full((rows - 1, cols), 1.0)
    wv[:, 0] = wv[:, -1] = 0.5
    dh = wh * (X[:, 1:] - X[:, :-1])
    dv = wv * (X[1:, :] - X[:-1, :])
    g[:, 1:] += dh
    g[:, :-1] -= dh
    g[1:, :] += dv
    g[:-1, :] -= dv
    g[:-1, :-1] += c0 * (X[:-1, :-1] ** 2 - 1.0) * X[:-1, :-1]
    return g.reshape(-1)


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_allen_cahn_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    rows = cols = 64
    n, c0, eps, cap = rows * cols, 4.0, 1e-6, 3000
    f = A.GridObjective(GR.ALLENCAHN, shape=(rows, cols), scalars=(c0,))
    x = _start(rows, cols)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(_allencahn_grad(x, rows, cols, c0)))
    else:
        lb, ub = np.full(n, -0.5), np.full(n, 0.9)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        x = np.clip(x, lb, ub)
        niter, fx = s.minimize(f, x, lb, ub)
        g = _allencahn_grad(x, rows, cols, c0)
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.any(x == 0.9)  # the wells are at +-1, outside the box: bounds are active
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    print("%s: niter %d nfev %d fx %.9g stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, measure, bound))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound


# ---------------------------------------------------------------- launch accounting
def _row_pair_pair(A, rows, cols):
    """the row-wise pair objective as a chain and as a grid (test_row_wise_grid_is_the_chain_of_the_same_body: equal values
    and gradients, so both solves take the same path); a chain costs the launches of a built-in (test_chain_objective_gpu)"""
    rng = np.random.default_rng(rows * cols)
    p0 = (0.5 + rng.random((rows, cols)))
    p0[:, -1] = 0
    p0[-1, :] = 0
    p0 = p0.reshape(-1)
    x0 = 0.5 * rng.standard_normal(rows * cols)
    return x0, (("chain", A.ChainObjective(GR.ROW_PAIR_CHAIN, K=2, data=(p0,))),
                ("grid", A.GridObjective(GR.ROW_PAIR_GRID, shape=(rows, cols), data=(p0,))))


def test_grid_solve_issues_the_launches_of_a_chain_solve(A):
    core, _ = A.load()
    rows, cols, m, iters = 400, 500, 6, 20
    x0, objs = _row_pair_pair(A, rows, cols)
    out = {}
    for name, f in objs:
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
        s.prepare(rows * cols)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x)
        c1 = _counters(core)
        out[name] = (niter, s.last.nfev, fx, c1[0] - c0[0])
    print(out)
    assert out["grid"] == out["chain"] and out["grid"][3] > 0 and out["grid"][0] == iters


def test_lbfgsb_grid_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    rows, cols, m, iters = 100, 200, 6, 25
    n = rows * cols
    x0, objs = _row_pair_pair(A, rows, cols)
    lb, ub = np.full(n, -0.5), np.full(n, 0.9)
    x0 = np.clip(x0, lb, ub)
    out = {}
    for name, f in objs:
        s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x, lb, ub)
        c1 = _counters(core)
        ahead = (C.c_int64 * 2)()
        assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
        out[name] = (niter, s.last.nfev, fx, c1[0] - c0[0], ahead[0], ahead[1])
    print(out)
    assert out["grid"][4] > 0 and out["grid"][5] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["grid"] == out["chain"]


# ---------------------------------------------------------------- refusals
def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    f = A.GridObjective(GR.ALLENCAHN, shape=(20, 50), scalars=(1.0,))
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, _start(20, 50))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, _start(20, 50))
    batch = B.LockstepBatch(A.LBFGSParam(m=3, max_iterations=3), 64, 2, dtype=np.float64)
    try:
        with pytest.raises(TypeError, match="fn must be callable"):
            batch.minimize_fn(A.GridObjective(GR.ALLENCAHN, shape=(8, 8)), np.zeros((2, 64)))
    finally:
        batch.close()
    with pytest.raises(ValueError, match="shape = \\(20, 50\\) does not multiply to n = 999"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(999))
