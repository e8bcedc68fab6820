"""-m gpu: periodic grid and volume objectives (lbfgspp_amd.PeriodicGridObjective, PeriodicVolumeObjective;
csrc/periodic_grid_kernels.cuh, csrc/periodic_volume_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/periodic_ref.py -- gradient and written x bit for bit, f
    and the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * cross-checks that do not rest on the restatement: the mask 0 against the open forms' kernels, translation on a torus, a
    periodic volume that ignores the slab below against the periodic grid of the stacked rows;
  * the periodic Allen-Cahn energy follows the reference (tests/golden/periodic_golden.json), from Python and from C++;
  * a 16 x 16 x 16 torus converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import grid_ref as GR
import oracle_lib as O
import periodic_ref as PR
import statement_ref as R
import volume_ref as VR
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates of a 16-byte pack
TRIAL_U = {2: 2, 3: 1}       # kGridTrialU, kVolumeTrialU: the tile depth of the two trial kernels
# above 2 * 1024 tiles every block walks its stride twice, and the stride is no multiple of cols or of rows*cols, so advance and
# retreat carry through the row and the slab seams: the volume test's shapes and their 2-D analogues (a grid tile is 512 packs)
WRAP = {(3, O.F64): ((9, 341, 342), (9, 341, 343)), (3, O.F32): ((9, 483, 484), (9, 483, 485)),
        (2, O.F64): ((6138, 342), (6138, 343)), (2, O.F32): ((8694, 484), (8694, 485))}
MIXED = {2: 1, 3: 2}  # the mixed mask of the large shapes: the grid's columns only, the volume's rows only


def _small(nd, dtype):
    """every mask is run at these"""
    W = PACK[dtype]
    if nd == 2:
        return [(2, 2), (2, 3), (3, 2), (3, 5)] + [(3, cols) for cols in (W - 1, W, W + 1, 2 * W + 1) if cols >= 2]
    return [(2, 2, 2), (2, 3, 2), (3, 2, 3), (3, 4, 5), (3, 3, 6), (3, 4, 3)]


def _large(nd, dtype):
    """the full mask and the mixed one are run at these"""
    W, U = PACK[dtype], TRIAL_U[nd]
    spans = tuple(c for span in (64 * W, 256 * W, U * 256 * W) for c in (span - W, span, span + 1, span + W))
    spans = tuple(dict.fromkeys(spans))
    if nd == 2:
        shapes = [(3, cols) for cols in spans]
        # the same spans reached by rows*cols with cols in {2, 3}: a row seam falls inside a wave, a block, a tile
        shapes += [(32 * W, 2), ((64 * W) // 3 + 1, 3), (128 * W, 2), ((256 * W) // 3 + 1, 3), (U * 128 * W, 2), ((U * 256 * W) // 3 + 1, 3)]
        shapes += [(4099, 2), (2, 4099), (3, 43)]  # thin in each direction; a flat tail
    else:
        shapes = [(2, 3, cols) for cols in spans]
        shapes += [(3, 32 * W, 2), (3, (64 * W) // 3 + 1, 3), (3, 128 * W, 2), (3, (256 * W) // 3 + 1, 3), (3, (256 * W) // 5, 5)]
        shapes += [(4099, 2, 2), (2, 4099, 2), (2, 2, 43)]
    return shapes + list(WRAP[(nd, dtype)])


def _cases():
    out = []
    for nd in (2, 3):
        for dtype in (O.F64, O.F32):
            full = 2 ** nd - 1
            todo = [(s, tuple(range(full + 1))) for s in _small(nd, dtype)] + [(s, (full, MIXED[nd])) for s in _large(nd, dtype)]
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
_COMPILE = {"grid": "lbfgsx_objective_compile_grid", "volume": "lbfgsx_objective_compile_volume",
            "pgrid": "lbfgsx_objective_compile_grid_periodic", "pvolume": "lbfgsx_objective_compile_volume_periodic"}


def _compile(c, body, form):
    key = (body, c.dtype, form)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = getattr(c.core, _COMPILE[form])(C.byref(h), c.dtype, body.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _bind_periodic(c, h, shape, mask, ptrs, cs):
    oid = C.c_int(-1)
    fn = c.core.lbfgsx_objective_bind_grid_periodic if len(shape) == 2 else c.core.lbfgsx_objective_bind_volume_periodic
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
    """the all-corners body with random per-node weights, uploaded once per context and bound per mask"""

    def __init__(self, c, shape, rng, scalars=None):
        self.c, self.shape, nd = c, tuple(shape), len(shape)
        assert c.n == int(np.prod(shape))
        self.p0 = (0.5 + rng.random(c.n)).astype(c.dt)
        self.ptrs = _upload(c, self.p0)
        self.scalars = (GR.ASYM_SCALARS if nd == 2 else VR.ASYM_SCALARS) if scalars is None else scalars
        self.cs = (C.c_double * 8)(*(tuple(self.scalars) + (0.0,) * (8 - nd)))
        self.h = _compile(c, PR.PASYM4 if nd == 2 else PR.PASYM8, "pgrid" if nd == 2 else "pvolume")
        self.terms = PR.pasym4_terms if nd == 2 else PR.pasym8_terms
        self._memo = {}

    def bind(self, mask):
        self.mask = mask
        return _bind_periodic(self.c, self.h, self.shape, mask, self.ptrs, self.cs)

    def ref(self, x, key=None):
        """(g, the existing cells' values) at x under the bound mask; the terms are computed once per key"""
        if key is None or key not in self._memo:
            t = self.terms(x, self.shape, self.p0, self.scalars)
            if key is None:
                return PR.periodic_grad(t[0], self.shape, self.mask), PR.values(t[1], self.shape, self.mask)
            self._memo[key] = t
        tg, v = self._memo[key]
        return PR.periodic_grad(tg, self.shape, self.mask), PR.values(v, self.shape, self.mask)


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


def _bound_cases(rng, n, dt, mask, full):
    """every case under the full mask of a small problem, one otherwise"""
    cases = R.bound_cases(rng, n, dt)
    return cases if (n <= 2000 and mask == full) else {"mixed_one_sided": cases["mixed_one_sided"]}


@pytest.mark.parametrize("dtype,shape,masks", _cases())
def test_b_eval_statement(A, dtype, shape, masks):
    n = int(np.prod(shape))
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, rng)
        for mask in masks:
            oid = f.bind(mask)
            for name, (x, _, lb, ub) in _bound_cases(rng, n, dt, mask, 2 ** len(shape) - 1).items():
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
            for name, (x, d, lb, ub) in _bound_cases(rng, n, dt, mask, 2 ** len(shape) - 1).items():
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
@pytest.mark.parametrize("shape", [(37, 131), (64, 256), (5, 7, 131), (9, 4, 40)], ids=lambda s: "x".join(map(str, s)))
def test_with_the_mask_zero_the_kernels_are_the_open_forms(A, dtype, shape):
    """the Allen-Cahn cell text (it reads neither j nor periodic) as a periodic objective with the mask 0 and as a GridObjective
    or VolumeObjective: the new kernels against the existing ones, g bit for bit and f equal"""
    n, nd = int(np.prod(shape)), len(shape)
    rng = np.random.default_rng(n)
    body = PR.ALLENCAHN if nd == 2 else PR.ALLENCAHN3
    with Ctx(A, dtype, n) as c:
        L = c.L
        c.up(L.VEC_X, rng.standard_normal(n).astype(c.dt))
        cs = (C.c_double * 8)(0.75, *([0.0] * 7))
        oid = C.c_int(-1)
        bind = c.core.lbfgsx_objective_bind_grid if nd == 2 else c.core.lbfgsx_objective_bind_volume
        L.check(bind(c.h, _compile(c, body, "grid" if nd == 2 else "volume"), *shape, None, C.byref(cs), C.byref(oid)))
        g_open, f_open = _eval(c, oid.value)
        g_per, f_per = _eval(c, _bind_periodic(c, _compile(c, body, "pgrid" if nd == 2 else "pvolume"), shape, 0, None, cs))
    _bits(g_per, g_open, "g")
    assert f_per == f_open and np.any(g_open != 0)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("shape,shift", [((7, 131), (2, 5)), ((5, 1027), (4, 1026)), ((3, 5, 67), (1, 4, 66)), ((4, 3, 130), (3, 1, 7))],
                         ids=lambda s: "x".join(map(str, s)))
def test_on_a_torus_the_gradient_of_the_rolled_x_is_the_rolled_gradient(A, dtype, shape, shift):
    """the all-corners body with its position scalars zero ignores position: on a full torus rolling x and p0 rolls the
    gradient bit for bit, whatever pack, wave and seam a node falls into (cols % W != 0 or not)"""
    n, nd = int(np.prod(shape)), len(shape)
    rng = np.random.default_rng(n)
    axes = tuple(range(nd))
    out = []
    x = rng.standard_normal(n)
    p0 = 0.5 + rng.random(n)
    for roll in (False, True):
        with Ctx(A, dtype, n) as c:
            xs, ps = (np.roll(a.reshape(shape), shift, axes).reshape(-1) if roll else a for a in (x, p0))
            ptrs = _upload(c, np.ascontiguousarray(ps, c.dt))
            c.up(c.L.VEC_X, xs.astype(c.dt))
            h = _compile(c, PR.PASYM4 if nd == 2 else PR.PASYM8, "pgrid" if nd == 2 else "pvolume")
            out.append(_eval(c, _bind_periodic(c, h, shape, 2 ** nd - 1, ptrs, None)))
    _bits(out[1][0], np.roll(out[0][0].reshape(shape), shift, axes).reshape(-1), "g of the rolled x")
    assert out[0][1] == out[1][1] and np.any(out[0][0] != 0)  # the same cells' values, summed order-independently


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("slabs,rows,cols", [(5, 7, 131), (9, 4, 40)])
def test_slab_wise_periodic_volume_is_the_periodic_grid_of_the_stacked_rows(A, dtype, slabs, rows, cols):
    """a cell body that ignores x[4..8), periodic in the column direction only, is the periodic grid objective of the same body on
    the slabs*rows x cols array of stacked rows, with a weight p0 that is zero where a grid cell would cross a slab end and on
    the last slab.  That is where the identity holds: a wrapped row or slab direction of the volume is no wrapped direction of
    the stacked grid.  Compared with == on values: dead partials and cut cells enter the sums as +-0."""
    n = slabs * rows * cols
    rng = np.random.default_rng(n)
    dt = NPDT[dtype]
    p0 = (0.5 + rng.random((slabs, rows, cols))).astype(dt)
    p0[-1] = 0
    p0[:, -1] = 0
    p0 = p0.reshape(-1)
    x = rng.standard_normal(n).astype(dt)
    with Ctx(A, dtype, n) as c:
        ptrs = _upload(c, p0)
        c.up(c.L.VEC_X, x)
        g2, f2 = _eval(c, _bind_periodic(c, _compile(c, VR.SLAB_GRID_2D, "pgrid"), (slabs * rows, cols), 1, ptrs, None))
        g3, f3 = _eval(c, _bind_periodic(c, _compile(c, VR.SLAB_GRID, "pvolume"), (slabs, rows, cols), 1, ptrs, None))
    assert np.array_equal(g2, g3) and f2 == f3
    assert np.any(g3 != 0) and np.all(g3.reshape(slabs, rows, cols)[-1] == 0)


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "periodic_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(shape):
    """tests/cpp/periodic_probe.cpp: start() -- a smooth bump scaled into the box [-0.5, 2], operation for operation; a grid is
    the single slab of a one-slab array (ts = 1/2)"""
    shape3 = (1,) * (3 - len(shape)) + tuple(shape)
    slabs, rows, cols = shape3
    ts = (np.arange(slabs, dtype=np.float64)[:, None, None] + 1.0) / float(slabs + 1)
    tr = (np.arange(rows, dtype=np.float64)[None, :, None] + 1.0) / float(rows + 1)
    tc = (np.arange(cols, dtype=np.float64)[None, None, :] + 1.0) / float(cols + 1)
    bump = ((ts * (1.0 - ts)) * (tr * (1.0 - tr))) * (tc * (1.0 - tc))
    return (-0.3 + (64.0 * bump) * (((1.0 + 0.5 * tr) + 0.25 * tc) + 0.125 * ts)).reshape(-1)


def _periodic_objective(A, shape, mask, c0):
    flags = tuple(bool(mask >> (len(shape) - 1 - ax) & 1) for ax in range(len(shape)))
    if len(shape) == 2:
        return A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, periodic=flags, scalars=(c0,))
    return A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=shape, periodic=flags, scalars=(c0,))


def _inst_id(i):
    return "%s-%s-mask%d" % (i["solver"], "x".join(map(str, i["shape"])), i["periodic"])


@pytest.mark.parametrize("inst", _golden()["instances"], ids=_inst_id)
def test_periodic_allen_cahn_follows_the_reference(A, inst):
    shape, tol = tuple(inst["shape"]), 1e-10
    n = int(np.prod(shape))
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(shape)
        f = _periodic_objective(A, shape, inst["periodic"], c0)
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


def test_cpp_periodic_objectives_follow_the_reference(tmp_path):
    """tests/cpp/periodic_probe.cpp with PeriodicGridObjective<double> and PeriodicVolumeObjective<double> in place of the
    functor, built with g++ against include/"""
    exe = str(tmp_path / "periodic_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DPERIODIC_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "periodic_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape, mask in sorted({(tuple(i["shape"]), i["periodic"]) for i in insts}):
        mine = [i for i in insts if (tuple(i["shape"]), i["periodic"]) == (shape, mask)]
        kmax = max(i["iterations"] for i in mine)
        shape3 = (0,) * (3 - len(shape)) + shape  # slabs = 0: a grid
        out = subprocess.run([exe] + [str(v) for v in shape3] + [str(mask), str(kmax)], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "PERIODIC PROBE OK" in out.stdout, out.stdout[-2000:]
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
    """the gradient of the torus Allen-Cahn energy in double, written independently of the body: every edge of the lattice has
    the weight 1/2 in total (four cells, an eighth each), every node is the origin of one cell"""
    X = x.reshape(shape)
    g = c0 * (X ** 2 - 1.0) * X
    for axis in range(len(shape)):
        g = g + (X - np.roll(X, 1, axis)) + (X - np.roll(X, -1, axis))
    return g.reshape(-1)


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_torus_allen_cahn_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    shape = (16, 16, 16)
    n, c0, eps, cap = 16 ** 3, 4.0, 1e-6, 3000
    f = A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=shape, scalars=(c0,))
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
    """_torus_gradient against tests/periodic_ref.py on a small torus (no device is used)"""
    shape = (3, 4, 5)
    x = np.random.default_rng(7).standard_normal(60)
    tg, _ = PR.allencahn3_terms(x, shape, 4.0)
    assert np.abs(_torus_gradient(x, shape, 4.0) - PR.periodic_grad(tg, shape, 7)).max() <= 1e-13


# ---------------------------------------------------------------- launch accounting
def _open_pair(A, shape):
    """the Allen-Cahn cell as the open form and as the periodic form with the mask 0
    (test_with_the_mask_zero_the_kernels_are_the_open_forms: equal values and gradients, so both solves take the same path)"""
    x0 = 0.5 * np.random.default_rng(int(np.prod(shape))).standard_normal(int(np.prod(shape)))
    none = (False,) * len(shape)
    if len(shape) == 2:
        return x0, (("open", A.GridObjective(PR.ALLENCAHN, shape=shape, scalars=(1.0,))),
                    ("periodic", A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, periodic=none, scalars=(1.0,))))
    return x0, (("open", A.VolumeObjective(PR.ALLENCAHN3, shape=shape, scalars=(1.0,))),
                ("periodic", A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=shape, periodic=none, scalars=(1.0,))))


@pytest.mark.parametrize("shape", [(400, 500), (20, 20, 500)], ids=["grid", "volume"])
def test_periodic_solve_issues_the_launches_of_an_open_solve(A, shape):
    core, _ = A.load()
    m, iters = 6, 20
    n = int(np.prod(shape))
    x0, objs = _open_pair(A, shape)
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
    assert out["periodic"] == out["open"] and out["periodic"][3] > 0 and out["periodic"][0] == iters


@pytest.mark.parametrize("shape", [(100, 200), (10, 10, 200)], ids=["grid", "volume"])
def test_lbfgsb_periodic_takes_the_fused_dg_maxstep_trial(A, shape):
    core, _ = A.load()
    m, iters = 6, 25
    n = int(np.prod(shape))
    x0, objs = _open_pair(A, shape)
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
    assert out["periodic"][4] > 0 and out["periodic"][5] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["periodic"] == out["open"]


def test_minimize_resident_takes_a_periodic_objective(A):
    """the start point uploaded into the device state, the result read back from it: the same solve as minimize()"""
    from lbfgspp_amd import _lib as L
    shape = (24, 40)
    n = 24 * 40
    prm = dict(m=6, epsilon=0, epsilon_rel=0, max_iterations=12)
    f = A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, scalars=(4.0,))
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
    for f, x0 in ((A.PeriodicGridObjective(PR.ALLENCAHN, shape=(20, 50), scalars=(1.0,)), _start((20, 50))),
                  (A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=(4, 5, 50), scalars=(1.0,)), _start((4, 5, 50)))):
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
