"""-m gpu: volume objectives (lbfgspp_amd.VolumeObjective, csrc/volume_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/volume_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * a volume objective whose cells ignore the slab below equals the grid objective of the same body on the stacked rows;
  * the Allen-Cahn energy follows the reference (tests/golden/volume_golden.json), from Python and from C++;
  * a 16 x 16 x 16 Allen-Cahn problem converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import statement_ref as R
import volume_ref as VR
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates of a 16-byte pack
TRIAL_U = 1                  # volume_kernels.cuh: kVolumeTrialU, the tile depth of the two trial kernels
# the capped grid is 1024 blocks and a tile of the trial kernels TRIAL_U * 256 = 256 packs: from 2 * 1024 tiles, that is above
# 2 * 1024 * 256 = 524288 packs (1048576 coordinates in f64, 2097152 in f32), every block walks its stride twice, and the
# stride of 1024 * 256 * W coordinates is no multiple of cols or of rows*cols, so advance and retreat carry through row and slab.
#   f64: 9 * 341 * 342 = 1049598 coordinates, 2050 tiles; cols and rows*cols even: both neighbours aligned
#        9 * 341 * 343 = 1052667 coordinates, 2056 tiles and a tail; cols and rows*cols odd: element loads
#   f32: 9 * 483 * 484 = 2103948 coordinates, 2055 tiles; cols = 4 * 121: both neighbours aligned
#        9 * 483 * 485 = 2108295 coordinates, 2059 tiles and a tail; cols and rows*cols odd: element loads
WRAP = {O.F64: ((9, 341, 342), (9, 341, 343)), O.F32: ((9, 483, 484), (9, 483, 485))}


def _shape_list(dtype):
    W = PACK[dtype]
    shapes = [(2, 2, 2), (2, 2, 3), (2, 3, 2), (3, 2, 2), (3, 4, 5), (4, 3, 2)]
    # cols around the pack: rows that straddle packs (cols = W - 1 = 1 is no volume in f64)
    shapes += [(slabs, rows, cols) for cols in (W - 1, W, W + 1, 2 * W + 1) if cols >= 2 for slabs, rows in ((2, 3), (3, 2))]
    # rows*cols odd (nothing aligned), = 2 mod 4 with cols odd and with cols even (f64: the slab neighbours aligned and the row
    # neighbours not, and both; f32: neither), a multiple of 4 with cols no multiple of 4 (f32: slab neighbours aligned, row
    # neighbours not).  cols % W == 0 implies rows*cols % W == 0: aligned rows over unaligned slabs do not exist
    shapes += [(3, 3, 5), (3, 2, 3), (3, 3, 6), (3, 4, 3), (3, 2, 6), (3, 3, 4)]
    spans = (64 * W - W, 64 * W, 64 * W + 1,                       # a wave's span
             256 * W - W, 256 * W + W,                             # a block's span
             TRIAL_U * 256 * W - W, TRIAL_U * 256 * W + W)         # a trial tile's span (the block's at depth 1)
    shapes += [(k, k, cols) for cols in spans for k in (2, 3)]
    # the same spans reached by rows*cols with cols small: a slab boundary falls inside a wave, a block, a tile
    shapes += [(3, 32 * W, 2), (3, (64 * W) // 3 + 1, 3), (3, 128 * W, 2), (3, (256 * W) // 3 + 1, 3), (3, (256 * W) // 5, 5)]
    shapes += [(4099, 2, 2), (2, 4099, 2), (2, 2, 43)]             # thin in each direction; a flat tail
    shapes += list(WRAP[dtype])
    return shapes


def _shapes():
    return [pytest.param(dtype, *shape, id="%s-%dx%dx%d" % (("f64" if dtype == O.F64 else "f32",) + shape))
            for dtype in (O.F64, O.F32) for shape in dict.fromkeys(_shape_list(dtype))]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, body, grid=False):
    key = (body, c.dtype, grid)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        fn = c.core.lbfgsx_objective_compile_grid if grid else c.core.lbfgsx_objective_compile_volume
        rc = fn(C.byref(h), c.dtype, body.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _bind(c, shape, rng):
    """compiles (once per process) and binds ASYM8 with random per-node weights; returns (id, x -> (g, cell values))"""
    L, n, dt = c.L, c.n, c.dt
    assert n == shape[0] * shape[1] * shape[2]
    p0 = (0.5 + rng.random(n)).astype(dt)
    ptrs = (C.c_void_p * 4)()
    dev = C.c_void_p()
    L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(*(VR.ASYM_SCALARS + (0.0,) * 5))
    oid = C.c_int(-1)
    L.check(c.core.lbfgsx_objective_bind_volume(c.h, _compile(c, VR.ASYM8), *shape, C.byref(ptrs), C.byref(cs), C.byref(oid)))
    assert oid.value == L.OBJ_BOUND
    s, r, cc = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert c.core.lbfgsx_objective_shape3(c.h, C.byref(s), C.byref(r), C.byref(cc)) == 0
    assert (s.value, r.value, cc.value) == tuple(shape)

    def ref(x):
        tg, v = VR.asym8_terms(x, *shape, p0)
        return VR.volume_grad(tg, *shape), v.reshape(-1)
    return oid.value, ref


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,slabs,rows,cols", _shapes())
def test_eval_statement(A, dtype, slabs, rows, cols):
    n = slabs * rows * cols
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, (slabs, rows, cols), rng)
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


@pytest.mark.parametrize("dtype,slabs,rows,cols", _shapes())
def test_trial_statement_in_both_tile_orders(A, dtype, slabs, rows, cols):
    n = slabs * rows * cols
    rng = np.random.default_rng(200 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, (slabs, rows, cols), rng)
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


@pytest.mark.parametrize("dtype,slabs,rows,cols", _shapes())
def test_b_eval_statement(A, dtype, slabs, rows, cols):
    n = slabs * rows * cols
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, (slabs, rows, cols), rng)
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


@pytest.mark.parametrize("dtype,slabs,rows,cols", _shapes())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, slabs, rows, cols):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    n = slabs * rows * cols
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        oid, ref = _bind(c, (slabs, rows, cols), rng)
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


# ---------------------------------------------------------------- a volume that ignores the slab below is a grid
def _slab_weights(rng, shape, dt):
    """per-node weights that are zero on the last slab and on the last row of every slab: the cells of the (slabs*rows, cols)
    grid that are no cell of the volume start there"""
    p0 = (0.5 + rng.random(shape)).astype(dt)
    p0[-1] = 0
    p0[:, -1] = 0
    return p0.reshape(-1)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("slabs,rows,cols", [(5, 7, 131), (9, 4, 40)])
def test_slab_wise_volume_is_the_grid_of_the_same_body(A, dtype, slabs, rows, cols):
    """a cell body that ignores x[4..8) is the grid objective of the same body on the slabs*rows x cols array of stacked rows,
    with a weight p0 that is zero where a grid cell would cross a slab end and on the last slab (no volume cell starts there):
    the new kernels against the existing ones.  The gradients are compared with == on values: the volume's dead partials and
    the grid's cut cells enter the sums as +-0, so a zero's sign may differ and nothing else."""
    n = slabs * rows * cols
    rng = np.random.default_rng(n)
    dt = NPDT[dtype]
    p0 = _slab_weights(rng, (slabs, rows, cols), dt)
    x = rng.standard_normal(n).astype(dt)
    got = {}
    with Ctx(A, dtype, n) as c:
        L = c.L
        ptrs = (C.c_void_p * 4)()
        dev = C.c_void_p()
        L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
        ptrs[0] = dev.value
        c.up(L.VEC_X, x)
        oid = C.c_int(-1)
        for name in ("grid", "volume"):
            if name == "grid":
                L.check(c.core.lbfgsx_objective_bind_grid(c.h, _compile(c, VR.SLAB_GRID_2D, grid=True), slabs * rows, cols,
                                                          C.byref(ptrs), None, C.byref(oid)))
            else:
                L.check(c.core.lbfgsx_objective_bind_volume(c.h, _compile(c, VR.SLAB_GRID), slabs, rows, cols, C.byref(ptrs), None,
                                                            C.byref(oid)))
            fx, g2, x2 = _d(3)
            L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
            got[name] = (c.down(L.VEC_G).copy(), fx.value)
    assert np.array_equal(got["grid"][0], got["volume"][0])
    assert np.any(got["volume"][0] != 0) and np.all(got["volume"][0].reshape(slabs, rows, cols)[-1] == 0)
    tg, _ = VR.slab_grid_terms(x, slabs, rows, cols, p0)
    assert np.array_equal(got["volume"][0], VR.volume_grad(tg, slabs, rows, cols))
    # the same terms, summed by the order-independent sum of both forms
    assert got["grid"][1] == got["volume"][1]


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "volume_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(slabs, rows, cols):
    """tests/cpp/volume_probe.cpp: start() -- a smooth bump scaled into the box [-0.5, 2], operation for operation"""
    ts = (np.arange(slabs, dtype=np.float64)[:, None, None] + 1.0) / float(slabs + 1)
    tr = (np.arange(rows, dtype=np.float64)[None, :, None] + 1.0) / float(rows + 1)
    tc = (np.arange(cols, dtype=np.float64)[None, None, :] + 1.0) / float(cols + 1)
    bump = ((ts * (1.0 - ts)) * (tr * (1.0 - tr))) * (tc * (1.0 - tc))
    return (-0.3 + (64.0 * bump) * (((1.0 + 0.5 * tr) + 0.25 * tc) + 0.125 * ts)).reshape(-1)


@pytest.mark.parametrize("inst", _golden()["instances"],
                         ids=lambda i: "%s-%dx%dx%d" % (i["solver"], i["slabs"], i["rows"], i["cols"]))
def test_allen_cahn_follows_the_reference(A, inst):
    shape, tol = (inst["slabs"], inst["rows"], inst["cols"]), 1e-10
    n = shape[0] * shape[1] * shape[2]
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(*shape)
        f = A.VolumeObjective(VR.ALLENCAHN3, shape=shape, scalars=(c0,))
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


def test_cpp_volume_objective_follows_the_reference(tmp_path):
    """tests/cpp/volume_probe.cpp with VolumeObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "volume_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DVOLUME_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "volume_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["slabs"], i["rows"], i["cols"]) for i in insts}):
        mine = [i for i in insts if (i["slabs"], i["rows"], i["cols"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe] + [str(v) for v in shape] + [str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert out.returncode == 0 and "VOLUME PROBE OK" in out.stdout, out.stdout[-2000:]
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
def _allencahn3_grad(x, shape, c0):
    """the gradient in double, written independently of the body: the edge Laplacian, an edge weighted by a quarter of the
    cells it belongs to (1, 2 or 4), plus the potential's derivative c0 (x^2 - 1) x on the nodes a cell starts at"""
    X = x.reshape(shape)
    g = np.zeros(shape)
    inner = [np.full(k, 2.0) for k in shape]  # per direction: the cells across that direction a node line touches
    for w in inner:
        w[0] = w[-1] = 1.0
    for axis in range(3):
        o1, o2 = [a for a in range(3) if a != axis]
        w = np.ones([shape[a] - (1 if a == axis else 0) for a in range(3)])
        for o in (o1, o2):
            view = [None, None, None]
            view[o] = slice(None)
            w = w * inner[o][tuple(view)]
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[axis], lo[axis] = slice(1, None), slice(None, -1)
        d = 0.25 * w * (X[tuple(hi)] - X[tuple(lo)])
        g[tuple(hi)] += d
        g[tuple(lo)] -= d
    core = X[:-1, :-1, :-1]
    g[:-1, :-1, :-1] += c0 * (core ** 2 - 1.0) * core
    return g.reshape(-1)


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_allen_cahn_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    shape = (16, 16, 16)
    n, c0, eps, cap = 16 ** 3, 4.0, 1e-6, 3000
    f = A.VolumeObjective(VR.ALLENCAHN3, shape=shape, scalars=(c0,))
    x = _start(*shape)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(_allencahn3_grad(x, shape, c0)))
    else:
        lb, ub = np.full(n, -0.5), np.full(n, 0.9)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        x = np.clip(x, lb, ub)
        niter, fx = s.minimize(f, x, lb, ub)
        g = _allencahn3_grad(x, shape, c0)
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.any(x == 0.9)  # the wells are at +-1, outside the box: bounds are active
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    print("%s: niter %d nfev %d fx %.9g stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, measure, bound))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound


def test_the_independent_gradient_is_the_restatement():
    """_allencahn3_grad against tests/volume_ref.py on a small volume (no device is used)"""
    shape = (3, 4, 5)
    x = np.random.default_rng(7).standard_normal(60)
    tg, _ = VR.allencahn3_terms(x, *shape, 4.0)
    assert np.abs(_allencahn3_grad(x, shape, 4.0) - VR.volume_grad(tg, *shape)).max() <= 1e-13


# ---------------------------------------------------------------- launch accounting
def _slab_pair(A, shape):
    """the slab-wise body as a grid and as a volume (test_slab_wise_volume_is_the_grid_of_the_same_body: equal values and
    gradients, so both solves take the same path)"""
    rng = np.random.default_rng(shape[0] * shape[1] * shape[2])
    p0 = _slab_weights(rng, shape, np.float64)
    x0 = 0.5 * rng.standard_normal(p0.size)
    return x0, (("grid", A.GridObjective(VR.SLAB_GRID_2D, shape=(shape[0] * shape[1], shape[2]), data=(p0,))),
                ("volume", A.VolumeObjective(VR.SLAB_GRID, shape=shape, data=(p0,))))


def test_volume_solve_issues_the_launches_of_a_grid_solve(A):
    core, _ = A.load()
    shape, m, iters = (20, 20, 500), 6, 20
    n = shape[0] * shape[1] * shape[2]
    x0, objs = _slab_pair(A, shape)
    out = {}
    for name, f in objs:
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x)
        c1 = _counters(core)
        out[name] = (niter, s.last.nfev, fx, c1[0] - c0[0])
    print(out)
    assert out["volume"] == out["grid"] and out["volume"][3] > 0 and out["volume"][0] == iters


def test_lbfgsb_volume_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    shape, m, iters = (10, 10, 200), 6, 25
    n = shape[0] * shape[1] * shape[2]
    x0, objs = _slab_pair(A, shape)
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
    assert out["volume"][4] > 0 and out["volume"][5] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["volume"] == out["grid"]


# ---------------------------------------------------------------- refusals
def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    f = A.VolumeObjective(VR.ALLENCAHN3, shape=(4, 5, 50), scalars=(1.0,))
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, _start(4, 5, 50))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, _start(4, 5, 50))
    batch = B.LockstepBatch(A.LBFGSParam(m=3, max_iterations=3), 64, 2, dtype=np.float64)
    try:
        with pytest.raises(TypeError, match="fn must be callable"):
            batch.minimize_fn(A.VolumeObjective(VR.ALLENCAHN3, shape=(4, 4, 4)), np.zeros((2, 64)))
    finally:
        batch.close()
    with pytest.raises(ValueError, match="shape = \\(4, 5, 50\\) does not multiply to n = 999"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(999))
