"""-m gpu: grid stencil objectives (lbfgspp_amd.StencilObjective; csrc/grid_stencil_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/stencil_ref.py -- gradient and written x bit for bit, f
    and the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * cross-checks that do not rest on the restatement: a 2x2 sub-body on a torus against the periodic grid kernels, a first-row
    body against the chain kernels row by row, translation on a torus, the interior of the open grid against the torus;
  * the plate energy follows the reference (tests/golden/stencil_golden.json), from Python and from C++;
  * a 32 x 32 torus converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import periodic_ref as PR
import statement_ref as R
import stencil_ref as SR
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates of a 16-byte pack
GRID_CAP, BLOCK, TRIAL_U = 1024, 256, 1  # kGridCap, kBlock, kStencilTrialU


def _small(dtype):
    """every mask is run at these.  rows = 3: the rows r-2 and r+1 coincide on a periodic axis; rows = 4: r-2 and r+2 do; rows =
    5: all five are distinct.  The columns: a pack inside a row, packs whose halo crosses the seam by one and by two on either
    side, a pack that fills the row, and a straddling pack in every residue of cols mod W"""
    W = PACK[dtype]
    cols = sorted({c for c in (3, W + 1, W + 2, 2 * W - 1, 2 * W, 2 * W + 1, 2 * W + 2, 3 * W + 1) if c >= 3})
    return [(rows, c) for rows in (3, 4, 5) for c in cols]


def _wrap(dtype):
    """the two smallest shapes with these column counts at which every block walks its stride twice: a capped launch has
    GRID_CAP blocks of one tile (BLOCK * U packs) each, so above 2 * GRID_CAP tiles every block takes a second tile; its stride,
    GRID_CAP tiles, is a power of two of nodes and no multiple of cols, so advance and retreat carry through the row seam"""
    W = PACK[dtype]
    nodes = 2 * GRID_CAP * BLOCK * TRIAL_U * W
    out = []
    for cols in ((342, 343) if dtype == O.F64 else (484, 485)):
        assert (GRID_CAP * BLOCK * TRIAL_U * W) % cols != 0
        out.append((nodes // cols + 1, cols))
    return out


def _large(dtype):
    """the full mask and the columns-only one are run at these"""
    W = PACK[dtype]
    shapes = []
    for span in (64 * W, 256 * W):  # one wave; one block = one tile at U = 1
        shapes += [(3, span + k) for k in (-W, -2, -1, 0, 1, 2, W)]
    shapes += [(32 * W, 4), (-(-64 * W // 3) + 1, 3)]  # row seams inside a wave
    shapes += [(4099, 3), (3, 4099), (3, 43)]  # thin in each direction; a flat tail
    return list(dict.fromkeys(shapes)) + _wrap(dtype)


def _cases():
    out = []
    for dtype in (O.F64, O.F32):
        todo = [(s, (0, 1, 2, 3)) for s in _small(dtype)] + [(s, (3, 1)) for s in _large(dtype)]
        for shape, masks in dict(todo).items():
            out.append(pytest.param(dtype, shape, masks, id="%s-%s" % ("f64" if dtype == O.F64 else "f32", "x".join(map(str, shape)))))
    return out


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, body, form="grid_stencil", K=None):
    key = (body, c.dtype, form, K)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        args = (c.dtype,) + (() if K is None else (K,))
        rc = getattr(c.core, "lbfgsx_objective_compile_" + form)(C.byref(h), *args, body.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _bind(c, h, shape, mask, ptrs, cs, form="grid_stencil"):
    oid = C.c_int(-1)
    fn = getattr(c.core, "lbfgsx_objective_bind_" + form)
    c.L.check(fn(c.h, h, *shape, mask, C.byref(ptrs) if ptrs is not None else None, C.byref(cs) if cs is not None else None,
                 C.byref(oid)))
    assert oid.value == c.L.OBJ_BOUND
    m = C.c_int(-1)
    assert c.core.lbfgsx_objective_periodic(c.h, C.byref(m)) == 0 and m.value == mask
    return oid.value


def _upload(c, p0):
    ptrs = (C.c_void_p * 4)()
    dev = C.c_void_p()
    c.L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
    ptrs[0] = dev.value
    return ptrs


class Asym:
    """the all-slots body with random per-node weights, uploaded once per context and bound per mask"""

    def __init__(self, c, shape, rng, scalars=SR.SASYM_SCALARS):
        self.c, self.shape = c, tuple(shape)
        assert c.n == int(np.prod(shape))
        self.p0 = (0.5 + rng.random(c.n)).astype(c.dt)
        self.ptrs = _upload(c, self.p0)
        self.scalars = scalars
        self.cs = (C.c_double * 8)(*(tuple(scalars) + (0.0,) * 6))
        self.h = _compile(c, SR.SASYM9)
        self._memo = {}

    def bind(self, mask):
        self.mask = mask
        return _bind(self.c, self.h, self.shape, mask, self.ptrs, self.cs)

    def ref(self, x, key=None):
        """(g, the existing patches' values) at x under the bound mask; the terms are computed once per key"""
        if key is None or key not in self._memo:
            t = SR.sasym9_terms(x, self.shape, self.p0, self.scalars)
            if key is None:
                return SR.stencil_grad(t[0], self.shape, self.mask), SR.values(t[1], self.shape, self.mask)
            self._memo[key] = t
        tg, v = self._memo[key]
        return SR.stencil_grad(tg, self.shape, self.mask), SR.values(v, self.shape, self.mask)


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,shape,masks", _cases())
def test_eval_statement(A, dtype, shape, masks):
    n = int(np.prod(shape))
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, rng)
        x = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, x)
        for mask in masks:
            oid = f.bind(mask)
            fx, g2, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g = c.down(L.VEC_G)
            g_ref, terms = f.ref(x, "x")
            _bits(g, g_ref, "mask %d: g" % mask)
            _sum_ok(fx.value, terms, dt, "mask %d: f" % mask)
            _dot_ok(g2.value, g_ref, g_ref, dt, "mask %d: g.g" % mask)
            _dot_ok(x2.value, x, x, dt, "mask %d: x.x" % mask)


@pytest.mark.parametrize("dtype,shape,masks", _cases())
def test_trial_statement_in_both_tile_orders(A, dtype, shape, masks):
    n = int(np.prod(shape))
    rng = np.random.default_rng(200 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, rng)
        xp = rng.standard_normal(n).astype(dt)
        d = rng.standard_normal(n).astype(dt)
        stale = np.full(n, -77.0, dt)
        step = 0.37
        xt_ref = R.axpy_ref(xp, d, step)
        for mask in masks:
            oid = f.bind(mask)
            c.up(L.VEC_X, xp)
            c.up(L.VEC_D, d)
            L.check(c.core.lbfgsx_ls_begin(c.h))
            g_ref, terms = f.ref(xt_ref, "xt")
            runs = []
            for k in range(2):
                c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible
                c.up(L.VEC_GT, stale)
                fx, dg = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                assert _launches(c.core) == before + 1
                xt, gt = c.down(L.VEC_XT), c.down(L.VEC_GT)
                _bits(xt, xt_ref, "mask %d launch %d: x trial" % (mask, k))
                _bits(gt, g_ref, "mask %d launch %d: g trial" % (mask, k))
                runs.append((fx.value, dg.value))
            _bits(c.down(L.VEC_XP), xp, "xp is left alone")
            assert runs[0] == runs[1], "f or g.d depends on the tile order"
            _sum_ok(runs[0][0], terms, dt, "mask %d: f" % mask)
            _dot_ok(runs[0][1], g_ref, d, dt, "mask %d: g.d" % mask)


def _bound_cases(rng, n, dt, mask):
    """every case under the full mask of a small problem, one otherwise"""
    cases = R.bound_cases(rng, n, dt)
    return cases if (n <= 2000 and mask == 3) else {"mixed_one_sided": cases["mixed_one_sided"]}


@pytest.mark.parametrize("dtype,shape,masks", _cases())
def test_b_eval_statement(A, dtype, shape, masks):
    n = int(np.prod(shape))
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, rng)
        for mask in masks:
            oid = f.bind(mask)
            for name, (x, _, lb, ub) in _bound_cases(rng, n, dt, mask).items():
                c.up(L.VEC_X, x)
                c.up(L.VEC_LB, lb)
                c.up(L.VEC_UB, ub)
                fx, pg, x2 = _d(3)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
                assert _launches(c.core) == before + 1
                g = c.down(L.VEC_G)
                g_ref, terms = f.ref(x)
                what = "mask %d %s" % (mask, name)
                _bits(g, g_ref, what + ": g")
                _sum_ok(fx.value, terms, dt, what + ": f")
                _dot_ok(x2.value, x, x, dt, what + ": x.x")
                assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), what


@pytest.mark.parametrize("dtype,shape,masks", _cases())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, shape, masks):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    n = int(np.prod(shape))
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, rng)
        for mask in masks:
            oid = f.bind(mask)
            for name, (x, d, lb, ub) in _bound_cases(rng, n, dt, mask).items():
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
                g_ref, terms = f.ref(xt_ref)
                what = "mask %d %s" % (mask, name)
                _bits(c.down(L.VEC_XT), xt_ref, what + ": x trial left by the fused pass")
                _bits(c.down(L.VEC_GT), g_ref, what + ": g trial left by the fused pass")
                fx, dgt = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
                assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)
                _bits(c.down(L.VEC_G), g0, what + ": g at xp is left alone")
                _dot_ok(dg.value, g0, d, dt, what + ": g.d")
                assert sm.value == R.step_max_ref(x, d, lb, ub), what
                _sum_ok(fx.value, terms, dt, what + ": f")
                _dot_ok(dgt.value, g_ref, d, dt, what + ": grad(x).d")


# ---------------------------------------------------------------- cross-checks that do not rest on the restatement
def _eval(c, oid):
    fx, g2, x2 = _d(3)
    c.L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
    return c.down(c.L.VEC_G).copy(), fx.value


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("shape", [(37, 131), (64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_a_2x2_sub_body_on_a_torus_is_the_periodic_grid_objective(A, dtype, shape):
    """the all-corners 2x2 text on the slots {0, 1, 3, 4} of a patch, T(0) in the other five g: on a full torus every node has the
    contributions of the periodic grid form in its order, behind and between zeros that change no bit"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    with Ctx(A, dtype, n) as c:
        ptrs = _upload(c, (0.5 + rng.random(n)).astype(c.dt))
        c.up(c.L.VEC_X, rng.standard_normal(n).astype(c.dt))
        cs = (C.c_double * 8)(0.0625, -0.03125, *([0.0] * 6))
        g_per, f_per = _eval(c, _bind(c, _compile(c, PR.PASYM4, "grid_periodic"), shape, 3, ptrs, cs, "grid_periodic"))
        g_sub, f_sub = _eval(c, _bind(c, _compile(c, SR.SUB2X2 % PR.PASYM4), shape, 3, ptrs, cs))
    _bits(g_sub, g_per, "g")
    assert f_sub == f_per and np.all(g_per != 0)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
def test_a_first_row_body_is_a_chain_objective_on_every_row(A, dtype):
    """a body on the slots {0, 1, 2}, the rows periodic and the columns open: every patch row exists, a patch exists iff
    col < cols-2, and the gradient of row r is that of the K = 3 chain on that row alone"""
    rows, cols = 5, 131
    rng = np.random.default_rng(rows * cols)
    x = rng.standard_normal(rows * cols).astype(NPDT[dtype])
    with Ctx(A, dtype, rows * cols) as c:
        c.up(c.L.VEC_X, x)
        g_sten, f_sten = _eval(c, _bind(c, _compile(c, SR.ROW3), (rows, cols), 2, None, None))
    g_rows, f_rows = [], []
    with Ctx(A, dtype, cols) as c:
        oid = C.c_int(-1)
        c.L.check(c.core.lbfgsx_objective_bind(c.h, _compile(c, SR.CHAIN3, "chain", 3), None, None, C.byref(oid)))
        for r in range(rows):
            c.up(c.L.VEC_X, np.ascontiguousarray(x[r * cols:(r + 1) * cols]))
            g, f = _eval(c, oid.value)
            g_rows.append(g)
            f_rows.append(f)
    _bits(g_sten, np.concatenate(g_rows), "g")
    assert np.all(g_sten != 0)
    # f: the five chains' sums, each rounded once, against the one sum of all patches
    tol = 8 * (2.0 ** -52 if dtype == O.F64 else 2.0 ** -23) * sum(abs(v) for v in f_rows)
    assert abs(f_sten - sum(f_rows)) <= tol


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("shape,shift", [((7, 131), (2, 5)), ((5, 1027), (4, 1026))], ids=lambda s: "x".join(map(str, s)))
def test_on_a_torus_the_gradient_of_the_rolled_x_is_the_rolled_gradient(A, dtype, shape, shift):
    """the plate body reads neither data nor position: on a full torus rolling x rolls the gradient bit for bit, whatever pack,
    wave and seam a node falls into (cols % W != 0 or not)"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    out = []
    for roll in (False, True):
        with Ctx(A, dtype, n) as c:
            xs = np.roll(x.reshape(shape), shift, (0, 1)).reshape(-1) if roll else x
            c.up(c.L.VEC_X, xs.astype(c.dt))
            cs = (C.c_double * 8)(0.75, *([0.0] * 7))
            out.append(_eval(c, _bind(c, _compile(c, SR.PLATE), shape, 3, None, cs)))
    _bits(out[1][0], np.roll(out[0][0].reshape(shape), shift, (0, 1)).reshape(-1), "g of the rolled x")
    assert out[0][1] == out[1][1] and np.any(out[0][0] != 0)  # the same patches' values, summed order-independently


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("shape", [(7, 131), (9, 64)], ids=lambda s: "x".join(map(str, s)))
def test_away_from_the_sides_the_open_grid_has_the_bits_of_the_torus(A, dtype, shape):
    """a coordinate at least two nodes from every side has its nine patches under every mask: with the mask 0 it has the bits
    it has under the mask 3"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + 1)
    with Ctx(A, dtype, n) as c:
        f = Asym(c, shape, rng)
        c.up(c.L.VEC_X, rng.standard_normal(n).astype(c.dt))
        g0, _ = _eval(c, f.bind(0))
        g3, _ = _eval(c, f.bind(3))
    inner = (slice(2, shape[0] - 2), slice(2, shape[1] - 2))
    a, b = g0.reshape(shape)[inner], g3.reshape(shape)[inner]
    assert a.size > 0 and a.tobytes() == b.tobytes() and np.all(a != 0)
    assert np.any(g0 != g3)  # the sides differ


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "stencil_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(shape):
    """tests/cpp/stencil_probe.cpp: start() -- a smooth bump, operation for operation"""
    rows, cols = shape
    tr = (np.arange(rows, dtype=np.float64)[:, None] + 1.0) / float(rows + 1)
    tc = (np.arange(cols, dtype=np.float64)[None, :] + 1.0) / float(cols + 1)
    bump = (tr * (1.0 - tr)) * (tc * (1.0 - tc))
    return (-0.3 + (16.0 * bump) * ((1.0 + 0.5 * tr) + 0.25 * tc)).reshape(-1)


def _inst_id(i):
    return "%s-%s-mask%d" % (i["solver"], "x".join(map(str, i["shape"])), i["periodic"])


@pytest.mark.parametrize("inst", _golden()["instances"], ids=_inst_id)
def test_the_plate_energy_follows_the_reference(A, inst):
    shape, tol = tuple(inst["shape"]), 1e-10
    n = int(np.prod(shape))
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(shape)
        f = A.StencilObjective(SR.PLATE, shape=shape, periodic=inst["periodic"], scalars=(c0,))
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


def test_cpp_stencil_objective_follows_the_reference(tmp_path):
    """tests/cpp/stencil_probe.cpp with StencilObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "stencil_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DSTENCIL_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "stencil_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape, mask in sorted({(tuple(i["shape"]), i["periodic"]) for i in insts}):
        mine = [i for i in insts if (tuple(i["shape"]), i["periodic"]) == (shape, mask)]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe] + [str(v) for v in shape] + [str(mask), str(kmax)], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "STENCIL PROBE OK" in out.stdout, out.stdout[-2000:]
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
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], shape, mask, k)


# ---------------------------------------------------------------- convergence
def _torus_gradient(x, shape, c0):
    """the gradient of the torus plate energy in double, written independently of the body: every node is the centre of one
    patch, so f = sum 1/2 (Lap x)^2 + c0/4 (x^2 - 1)^2 and its gradient is Lap(Lap x) + c0 (x^2 - 1) x, Lap the symmetric
    five-point Laplacian"""
    X = x.reshape(shape)

    def lap(u):
        return np.roll(u, 1, 0) + np.roll(u, -1, 0) + np.roll(u, 1, 1) + np.roll(u, -1, 1) - 4.0 * u
    return (lap(lap(X)) + c0 * (X ** 2 - 1.0) * X).reshape(-1)


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_torus_plate_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    shape = (32, 32)
    n, c0, eps, cap = 32 * 32, 4.0, 1e-6, 3000
    f = A.StencilObjective(SR.PLATE, shape=shape, periodic=3, scalars=(c0,))
    x = _start(shape)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(_torus_gradient(x, shape, c0)))
    else:
        lb, ub = np.full(n, -0.5), np.full(n, 0.9)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        x = np.clip(x, lb, ub)
        niter, fx = s.minimize(f, x, lb, ub)
        g = _torus_gradient(x, shape, c0)
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.any(x == 0.9) or np.any(x == -0.5)  # the wells are at +-1, outside the box: bounds are active
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    print("%s: niter %d nfev %d fx %.9g stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, measure, bound))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound


def test_the_independent_gradient_is_the_restatement():
    """_torus_gradient against tests/stencil_ref.py on a small torus (no device is used)"""
    shape = (4, 5)
    x = np.random.default_rng(7).standard_normal(20)
    tg, _ = SR.plate_terms(x, shape, 4.0)
    assert np.abs(_torus_gradient(x, shape, 4.0) - SR.stencil_grad(tg, shape, 3)).max() <= 1e-12


# ---------------------------------------------------------------- launch accounting
def _pair(A, shape):
    """the Allen-Cahn cell as a periodic grid objective on the torus and as the 2x2 sub-body of a stencil objective
    (test_a_2x2_sub_body_on_a_torus_is_the_periodic_grid_objective: equal values and gradients, so both solves take the same
    path)"""
    n = int(np.prod(shape))
    x0 = 0.5 * np.random.default_rng(n).standard_normal(n)
    return x0, (("periodic", A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, scalars=(1.0,))),
                ("stencil", A.StencilObjective(SR.SUB2X2 % PR.ALLENCAHN, shape=shape, periodic=3, scalars=(1.0,))))


def test_a_stencil_solve_issues_the_launches_of_a_periodic_grid_solve(A):
    core, _ = A.load()
    m, iters = 6, 20
    shape = (400, 500)
    n = int(np.prod(shape))
    x0, objs = _pair(A, shape)
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
    assert out["stencil"] == out["periodic"] and out["stencil"][3] > 0 and out["stencil"][0] == iters


def test_lbfgsb_stencil_takes_the_fused_dg_maxstep_trial(A):
    """every first trial of an iteration rides on lbfgsx_b_dg_maxstep_trial, as many as the periodic grid form's, and its trial
    is taken over"""
    core, _ = A.load()
    m, iters = 6, 25
    shape = (100, 200)
    n = int(np.prod(shape))
    x0, objs = _pair(A, shape)
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
    assert out["stencil"][4] > 0 and out["stencil"][5] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["stencil"][4] >= out["stencil"][0]           # one per iteration
    assert out["stencil"] == out["periodic"]


def test_minimize_resident_takes_a_stencil_objective(A):
    """the start point uploaded into the device state, the result read back from it: the same solve as minimize()"""
    from lbfgspp_amd import _lib as L
    shape = (24, 40)
    n = 24 * 40
    prm = dict(m=6, epsilon=0, epsilon_rel=0, max_iterations=12)
    f = A.StencilObjective(SR.PLATE, shape=shape, periodic=1, scalars=(4.0,))
    x = _start(shape)
    s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
    want = s.minimize(f, x)
    core, _ = A.load()
    s2 = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
    h = s2.prepare(n)
    x0 = _start(shape)
    L.check(core.lbfgsx_upload(h, L.VEC_X, x0.ctypes.data_as(C.c_void_p)))
    assert s2.minimize_resident(f, n) == want
    got = np.empty(n)
    L.check(core.lbfgsx_download(h, L.VEC_X, got.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(got, x)


# ---------------------------------------------------------------- refusals
def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    f, x0 = A.StencilObjective(SR.PLATE, shape=(20, 50), scalars=(1.0,)), _start((20, 50))
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, x0.copy())
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, x0.copy())
    with pytest.raises(ValueError, match="does not multiply to n = 999"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(999))
