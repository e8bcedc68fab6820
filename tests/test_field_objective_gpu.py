"""-m gpu: grid field objectives (lbfgspp_amd.GridFieldObjective; csrc/grid_field_kernels.cuh) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/field_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal;
  * cross-checks that do not rest on the restatement: D = 1 against the periodic grid kernels, the open grid against the mesh
    kernels on the quad mesh, translation on a torus, uncoupled components against the periodic grid kernels per component;
  * the Ginzburg-Landau energy follows the reference (tests/golden/field_golden.json), from Python and from C++;
  * a 32 x 32 torus of two components converges under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import oracle_lib as O
import periodic_ref as PR
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the nodes a thread owns
GRID_CAP, BLOCK = 1024, 256  # kGridCap, kBlock: the blocks of a launch are capped, a block has 256 threads


def _trial_u(D):
    """GridFieldFamily::U: the tile depth of the two trial kernels, in node packs per thread"""
    return 2 if D == 1 else 1


def _small(dtype):
    """every mask is run at these: a pack inside a row, a pack that ends at the seam, a straddling pack, and with D both
    alignment classes of (cols*D) % W"""
    W = PACK[dtype]
    return [(2, 2), (2, 3), (3, 2), (3, 5)] + [(3, cols) for cols in (W - 1, W, W + 1, 2 * W + 1) if cols >= 2]


def _wrap(dtype, D):
    """the two smallest shapes with these column counts at which every block walks its stride twice: a capped launch has
    GRID_CAP blocks of one tile (BLOCK * U node packs) each, so above 2 * GRID_CAP tiles of node packs every block takes a second
    tile; its stride, GRID_CAP tiles, is a power of two of nodes and no multiple of cols, so advance and retreat carry through
    the row seam"""
    W = PACK[dtype]
    nodes = 2 * GRID_CAP * BLOCK * _trial_u(D) * W
    out = []
    for cols in ((342, 343) if dtype == O.F64 else (484, 485)):
        assert (GRID_CAP * BLOCK * _trial_u(D) * W) % cols != 0
        out.append((nodes // cols + 1, cols))
    return out


def _large(dtype, D):
    """the full mask and the column-periodic one are run at these"""
    W, U = PACK[dtype], _trial_u(D)
    spans = tuple(c for span in (64 * W, 256 * W, U * 256 * W) for c in (span - W, span, span + 1, span + W))
    shapes = [(3, cols) for cols in dict.fromkeys(spans)]
    shapes += [(32 * W, 2), ((64 * W) // 3 + 1, 3)]  # a row seam inside a wave
    shapes += [(4099, 2), (2, 4099), (3, 43)]        # thin in each direction; a flat tail
    return shapes + _wrap(dtype, D)


def _cases():
    out = []
    for dtype in (O.F64, O.F32):
        for D in (1, 2, 3):
            todo = [(s, (0, 1, 2, 3)) for s in _small(dtype)]
            if D >= 2:
                todo += [(s, (3, 1)) for s in _large(dtype, D)]
            for shape, masks in dict(todo).items():
                out.append(pytest.param(dtype, shape, D, masks,
                                        id="%s-D%d-%s" % ("f64" if dtype == O.F64 else "f32", D, "x".join(map(str, shape)))))
    return out


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, body, D):
    """D = 0: the body as a periodic grid objective"""
    key = (body, c.dtype, D)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        if D:
            rc = c.core.lbfgsx_objective_compile_grid_field(C.byref(h), c.dtype, D, body.encode(), log, len(log))
        else:
            rc = c.core.lbfgsx_objective_compile_grid_periodic(C.byref(h), c.dtype, body.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _bind_field(c, h, shape, mask, ptrs, cs):
    oid = C.c_int(-1)
    c.L.check(c.core.lbfgsx_objective_bind_grid_field(c.h, h, *shape, mask, C.byref(ptrs) if ptrs is not None else None,
                                                      C.byref(cs) if cs is not None else None, C.byref(oid)))
    assert oid.value == c.L.OBJ_BOUND
    m, r, cc = C.c_int(-1), C.c_int64(0), C.c_int64(0)
    assert c.core.lbfgsx_objective_periodic(c.h, C.byref(m)) == 0 and m.value == mask
    assert c.core.lbfgsx_objective_shape(c.h, C.byref(r), C.byref(cc)) == 0 and (r.value, cc.value) == tuple(shape)
    return oid.value


def _bind_periodic(c, h, shape, mask, ptrs, cs):
    oid = C.c_int(-1)
    c.L.check(c.core.lbfgsx_objective_bind_grid_periodic(c.h, h, *shape, mask, C.byref(ptrs) if ptrs is not None else None,
                                                         C.byref(cs) if cs is not None else None, C.byref(oid)))
    assert oid.value == c.L.OBJ_BOUND
    return oid.value


def _upload(c, p0):
    ptrs = (C.c_void_p * 4)()
    dev = C.c_void_p()
    c.L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, p0.ctypes.data_as(C.c_void_p), p0.size, C.byref(dev)))
    ptrs[0] = dev.value
    return ptrs


class Asym:
    """the all-corners body with random per-coordinate weights, uploaded once per context and bound per mask"""

    def __init__(self, c, shape, D, rng, scalars=FR.FASYM_SCALARS):
        self.c, self.shape, self.D = c, tuple(shape), D
        assert c.n == shape[0] * shape[1] * D
        self.p0 = (0.5 + rng.random(c.n)).astype(c.dt)
        self.ptrs = _upload(c, self.p0)
        self.scalars = scalars
        self.cs = (C.c_double * 8)(*(tuple(scalars) + (0.0,) * 6))
        self.h = _compile(c, FR.FASYM, D)
        assert c.core.lbfgsx_objective_D(self.h) == D and c.core.lbfgsx_objective_K(self.h) == 4
        self._memo = {}

    def bind(self, mask):
        self.mask = mask
        return _bind_field(self.c, self.h, self.shape, mask, self.ptrs, self.cs)

    def ref(self, x, key=None):
        """(g, the existing cells' values) at x under the bound mask; the terms are computed once per key"""
        if key is None or key not in self._memo:
            t = FR.fasym_terms(x, self.shape, self.D, self.p0, self.scalars)
            if key is None:
                return FR.field_grad(t[0], self.shape, self.D, self.mask), FR.values(t[1], self.shape, self.mask)
            self._memo[key] = t
        tg, v = self._memo[key]
        return FR.field_grad(tg, self.shape, self.D, self.mask), FR.values(v, self.shape, self.mask)


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,shape,D,masks", _cases())
def test_eval_statement(A, dtype, shape, D, masks):
    n = shape[0] * shape[1] * D
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, D, rng)
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


@pytest.mark.parametrize("dtype,shape,D,masks", _cases())
def test_trial_statement_in_both_tile_orders(A, dtype, shape, D, masks):
    n = shape[0] * shape[1] * D
    rng = np.random.default_rng(200 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, D, rng)
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


@pytest.mark.parametrize("dtype,shape,D,masks", _cases())
def test_b_eval_statement(A, dtype, shape, D, masks):
    n = shape[0] * shape[1] * D
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, D, rng)
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


@pytest.mark.parametrize("dtype,shape,D,masks", _cases())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, shape, D, masks):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    n = shape[0] * shape[1] * D
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        f = Asym(c, shape, D, rng)
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
def _eval_and_two_trials(c, oid):
    """g, f, g.g, x.x of lbfgsx_eval and, in both tile orders, the g, x, f and g.d of lbfgsx_trial: VEC_X and VEC_D are uploaded"""
    L = c.L
    fx, g2, x2 = _d(3)
    L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
    got = [c.down(L.VEC_G).copy(), fx.value, g2.value, x2.value]
    L.check(c.core.lbfgsx_ls_begin(c.h))
    for k in range(2):
        ft, dg = _d(2)
        L.check(c.core.lbfgsx_trial(c.h, oid, 0.37, C.byref(ft), C.byref(dg)))
        got += [c.down(L.VEC_GT).copy(), c.down(L.VEC_XT).copy(), ft.value, dg.value]
    return got


def _same(a, b, what):
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            _bits(v, u, what)
        else:
            assert u == v, what


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("shape", [(37, 131), (64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_with_one_unknown_per_node_the_kernels_are_the_periodic_grids(A, dtype, shape):
    """PASYM4 (every corner weighted through j) as a field with D = 1 and as a PeriodicGridObjective, under every mask: g, x, f
    and the sums bit-identical from lbfgsx_eval and both trial orders.  At the mask 0 that is the GridObjective too
    (tests/test_periodic_objective_gpu.py)"""
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n)
    with Ctx(A, dtype, n) as c:
        L = c.L
        c.up(L.VEC_X, rng.standard_normal(n).astype(c.dt))
        c.up(L.VEC_D, rng.standard_normal(n).astype(c.dt))
        ptrs = _upload(c, (0.5 + rng.random(n)).astype(c.dt))
        cs = (C.c_double * 8)(0.375, -0.625, *([0.0] * 6))
        for mask in range(4):
            want = _eval_and_two_trials(c, _bind_periodic(c, _compile(c, PR.PASYM4, 0), shape, mask, ptrs, cs))
            got = _eval_and_two_trials(c, _bind_field(c, _compile(c, PR.PASYM4, 1), shape, mask, ptrs, cs))
            _same(want, got, "mask %d: field against periodic grid" % mask)
            assert np.any(got[0] != 0)


# the element body of the quad mesh: FASYM after the lines that give the mesh form's arguments the field form's names
MESH_ALIAS = "const int64_t (&j)[4] = v;\nconst int64_t row = 0, col = 0;\n"


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("shape", [(7, 131), (5, 1027)], ids=lambda s: "x".join(map(str, s)))
def test_the_open_grid_is_the_quad_mesh_of_its_cells(A, dtype, D, shape):
    """mask 0 against MeshObjective with K = 4 and the same D on the quad mesh whose element e is the cell with the e-th origin
    in ascending order, nodes in corner order: a node's elements in ascending index are its cells in the field form's order,
    so g is bit-equal; f, the order-independent sum of the same values, is equal.  The position scalars are zero: the mesh
    body has no row and col"""
    rows, cols = shape
    n = rows * cols * D
    rng = np.random.default_rng(n)
    origin = (np.arange(rows - 1)[:, None] * cols + np.arange(cols - 1)[None, :]).reshape(-1)
    el = np.ascontiguousarray(np.stack([origin, origin + 1, origin + cols, origin + cols + 1], 1), np.int32)
    with Ctx(A, dtype, n) as c:
        L = c.L
        c.up(L.VEC_X, rng.standard_normal(n).astype(c.dt))
        c.up(L.VEC_D, rng.standard_normal(n).astype(c.dt))
        ptrs = _upload(c, (0.5 + rng.random(n)).astype(c.dt))
        got = _eval_and_two_trials(c, _bind_field(c, _compile(c, FR.FASYM, D), shape, 0, ptrs, None))
        hm = C.c_void_p()
        log = C.create_string_buffer(8192)
        assert c.core.lbfgsx_objective_compile_mesh(C.byref(hm), dtype, 4, D, None, (MESH_ALIAS + FR.FASYM).encode(), log,
                                                    len(log)) == 0, log.value.decode()
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind_mesh(c.h, hm, el.shape[0], el.ctypes.data_as(C.c_void_p), 0, C.byref(ptrs), None,
                                                  C.byref(oid)))
        want = _eval_and_two_trials(c, oid.value)
        c.core.lbfgsx_objective_destroy(hm)
    _same(want, got, "field against mesh")
    assert np.any(got[0] != 0)


def _eval(c, oid):
    fx, g2, x2 = _d(3)
    c.L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
    return c.down(c.L.VEC_G).copy(), fx.value


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("shape,shift", [((7, 131), (2, 5)), ((5, 1027), (4, 1026))], ids=lambda s: "x".join(map(str, s)))
def test_on_a_torus_the_gradient_of_the_rolled_x_is_the_rolled_gradient(A, dtype, D, shape, shift):
    """the all-corners body with its position scalars zero ignores position: on a full torus rolling x and p0 by whole nodes
    rolls the gradient bit for bit, whatever pack, wave and seam a node falls into"""
    n = shape[0] * shape[1] * D
    rng = np.random.default_rng(n)
    full = tuple(shape) + (D,)
    out = []
    x = rng.standard_normal(n)
    p0 = 0.5 + rng.random(n)
    for roll in (False, True):
        with Ctx(A, dtype, n) as c:
            xs, ps = (np.roll(a.reshape(full), shift, (0, 1)).reshape(-1) if roll else a for a in (x, p0))
            ptrs = _upload(c, np.ascontiguousarray(ps, c.dt))
            c.up(c.L.VEC_X, xs.astype(c.dt))
            out.append(_eval(c, _bind_field(c, _compile(c, FR.FASYM, D), shape, 3, ptrs, None)))
    _bits(out[1][0], np.roll(out[0][0].reshape(full), shift, (0, 1)).reshape(-1), "g of the rolled x")
    assert out[0][1] == out[1][1] and np.any(out[0][0] != 0)  # the same cells' values, summed order-independently


# D copies of the Allen-Cahn cell (grid_ref.ALLENCAHN, statement by statement, per component): no component sees another
UNCOUPLED = """T v = T(0);
#pragma unroll
for (int d = 0; d < D; d++)
{
    const T a = x[D + d] - x[d];
    const T b = x[2 * D + d] - x[d];
    const T e = x[3 * D + d] - x[2 * D + d];
    const T h = x[3 * D + d] - x[D + d];
    const T u = x[d] * x[d] - T(1);
    const T k = c[0] * T(0.25);
    g[d] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[d]);
    g[D + d] = T(0.5) * (a - h);
    g[2 * D + d] = T(0.5) * (b - e);
    g[3 * D + d] = T(0.5) * (e + h);
    v = v + (T(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u));
}
return v;"""


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("shape,mask", [((7, 131), 3), ((5, 1027), 1), ((37, 64), 2), ((9, 130), 0)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else "mask%d" % s)
def test_uncoupled_components_are_the_periodic_grid_of_each_plane(A, dtype, D, shape, mask):
    """per component the gradient is that of PeriodicGridObjective with the Allen-Cahn text on the component's plane, bit for
    bit: the field kernels' windows, seams and order against the scalar kernels'"""
    N = shape[0] * shape[1]
    rng = np.random.default_rng(N * D + mask)
    x = rng.standard_normal(N * D).astype(NPDT[dtype])
    cs = (C.c_double * 8)(0.75, *([0.0] * 7))
    with Ctx(A, dtype, N * D) as c:
        c.up(c.L.VEC_X, x)
        g, _ = _eval(c, _bind_field(c, _compile(c, UNCOUPLED, D), shape, mask, None, cs))
    g = g.reshape(N, D)
    with Ctx(A, dtype, N) as c:
        for d in range(D):
            c.up(c.L.VEC_X, np.ascontiguousarray(x.reshape(N, D)[:, d]))
            plane, _ = _eval(c, _bind_periodic(c, _compile(c, PR.ALLENCAHN, 0), shape, mask, None, cs))
            _bits(np.ascontiguousarray(g[:, d]), plane, "component %d" % d)
            assert np.any(plane != 0)


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "field_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(shape, D):
    """tests/cpp/field_probe.cpp: start(), operation for operation"""
    rows, cols = shape
    tr = (np.arange(rows, dtype=np.float64)[:, None, None] + 1.0) / float(rows + 1)
    tc = (np.arange(cols, dtype=np.float64)[None, :, None] + 1.0) / float(cols + 1)
    td = (np.arange(D, dtype=np.float64)[None, None, :] + 1.0) / float(D + 1)
    bump = (tr * (1.0 - tr)) * (tc * (1.0 - tc))
    return (-0.3 + ((16.0 * bump) * (((1.0 + 0.5 * tr) + 0.25 * tc) + 0.125 * td)) * (1.0 - 0.5 * td)).reshape(-1)


def _flags(mask):
    return (bool(mask & 2), bool(mask & 1))


def _inst_id(i):
    return "%s-%s-D%d-mask%d" % (i["solver"], "x".join(map(str, i["shape"])), i["D"], i["periodic"])


@pytest.mark.parametrize("inst", _golden()["instances"], ids=_inst_id)
def test_ginzburg_landau_follows_the_reference(A, inst):
    shape, D, tol = tuple(inst["shape"]), inst["D"], 1e-10
    n = shape[0] * shape[1] * D
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(shape, D)
        f = A.GridFieldObjective(FR.GL, shape=shape, D=D, periodic=_flags(inst["periodic"]), scalars=(c0,))
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


def test_cpp_grid_field_objective_follows_the_reference(tmp_path):
    """tests/cpp/field_probe.cpp with GridFieldObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "field_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DFIELD_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "field_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape, D, mask in sorted({(tuple(i["shape"]), i["D"], i["periodic"]) for i in insts}):
        mine = [i for i in insts if (tuple(i["shape"]), i["D"], i["periodic"]) == (shape, D, mask)]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe] + [str(v) for v in shape + (D, mask, kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert out.returncode == 0 and "FIELD PROBE OK" in out.stdout, out.stdout[-2000:]
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
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], shape, D, mask, k)


# ---------------------------------------------------------------- convergence
def _torus_gradient(x, shape, D, c0):
    """the gradient of the torus Ginzburg-Landau energy in double, written independently of the body: every edge of the
    lattice has the weight 1/2 in total (two cells, a quarter each), every node is the origin of one cell"""
    X = x.reshape(tuple(shape) + (D,))
    g = c0 * ((X ** 2).sum(axis=2, keepdims=True) - 1.0) * X
    for axis in (0, 1):
        g = g + (X - np.roll(X, 1, axis)) + (X - np.roll(X, -1, axis))
    return g.reshape(-1)


def test_the_independent_gradient_is_the_restatement():
    """_torus_gradient against tests/field_ref.py on a small torus (no device is used)"""
    shape, D = (4, 5), 3
    x = np.random.default_rng(7).standard_normal(60)
    tg, _ = FR.gl_terms(x, shape, D, 4.0)
    assert np.abs(_torus_gradient(x, shape, D, 4.0) - FR.field_grad(tg, shape, D, 3)).max() <= 1e-13


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_torus_ginzburg_landau_converges(A, solver):
    """the solver ends by its own gradient test before max_iterations, and the gradient recomputed in numpy satisfies that
    test within a factor 2: ||g|| <= eps max(1, ||x||) for L-BFGS, ||P(x - g) - x||_inf <= eps max(1, ||x||) for L-BFGS-B"""
    shape, D = (32, 32), 2
    n, c0, eps, cap = 32 * 32 * 2, 4.0, 1e-6, 3000
    f = A.GridFieldObjective(FR.GL, shape=shape, D=D, periodic=(True, True), scalars=(c0,))
    x = _start(shape, D)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(_torus_gradient(x, shape, D, c0)))
    else:
        lb, ub = np.full(n, -0.25), np.full(n, 0.6)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        x = np.clip(x, lb, ub)
        niter, fx = s.minimize(f, x, lb, ub)
        g = _torus_gradient(x, shape, D, c0)
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.any(x == 0.6) or np.any(x == -0.25)  # the minima have |u| = 1, outside the box: bounds are active
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    print("%s: niter %d nfev %d fx %.9g stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, measure, bound))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound


# ---------------------------------------------------------------- launch accounting
def _same_n_pair(A, shape, D):
    """a field solve and a PeriodicGridObjective solve of the same n: the Allen-Cahn text on rows x (cols*D) nodes"""
    n = shape[0] * shape[1] * D
    x0 = 0.5 * np.random.default_rng(n).standard_normal(n)
    return x0, (("periodic", A.PeriodicGridObjective(PR.ALLENCAHN, shape=(shape[0], shape[1] * D), scalars=(1.0,))),
                ("field", A.GridFieldObjective(FR.GL, shape=shape, D=D, periodic=(True, True), scalars=(1.0,))))


def test_field_solve_issues_the_launches_of_a_periodic_grid_solve_of_the_same_n(A):
    """one text as a PeriodicGridObjective and as a field with D = 1 (equal values and gradients:
    test_with_one_unknown_per_node_the_kernels_are_the_periodic_grids), so both solves take the same path and must issue the
    same launches; a field of two components of the same n: one launch per evaluation, every iteration's other launches are
    the solver's own"""
    core, _ = A.load()
    m, iters, shape = 6, 20, (400, 500)
    n = shape[0] * shape[1]
    x0 = 0.5 * np.random.default_rng(n).standard_normal(n)
    out = {}
    for name, f in (("periodic", A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, scalars=(1.0,))),
                    ("field", A.GridFieldObjective(PR.ALLENCAHN, shape=shape, D=1, periodic=(True, True), scalars=(1.0,))),
                    ("field2", A.GridFieldObjective(FR.GL, shape=(400, 250), D=2, periodic=(True, True), scalars=(1.0,)))):
        s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
        s.prepare(n)
        x = x0.copy()
        c0 = _counters(core)
        niter, fx = s.minimize(f, x)
        c1 = _counters(core)
        out[name] = (niter, s.last.nfev, fx, c1[0] - c0[0])
    print(out)
    assert out["field"] == out["periodic"] and out["field"][3] > 0 and out["field"][0] == iters
    assert out["field2"][0] == iters and out["field2"][3] > out["field2"][1] > iters


def test_lbfgsb_field_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    m, iters, shape, D = 6, 25, (100, 100), 2
    n = shape[0] * shape[1] * D
    x0, objs = _same_n_pair(A, shape, D)
    lb, ub = np.full(n, -0.5), np.full(n, 0.9)
    x0 = np.clip(x0, lb, ub)
    f = dict(objs)["field"]
    s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
    s.prepare(n)
    x = x0.copy()
    niter, fx = s.minimize(f, x, lb, ub)
    ahead = (C.c_int64 * 2)()
    assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
    print(niter, s.last.nfev, fx, ahead[0], ahead[1])
    assert niter == iters and ahead[0] > 0 and ahead[1] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over


def test_minimize_resident_takes_a_field_objective(A):
    """the start point uploaded into the device state, the result read back from it: the same solve as minimize()"""
    from lbfgspp_amd import _lib as L
    shape, D = (24, 20), 3
    n = 24 * 20 * 3
    prm = dict(m=6, epsilon=0, epsilon_rel=0, max_iterations=12)
    f = A.GridFieldObjective(FR.GL, shape=shape, D=D, periodic=(True, False), scalars=(4.0,))
    x = _start(shape, D)
    s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
    want = s.minimize(f, x)
    core, _ = A.load()
    s2 = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
    h = s2.prepare(n)
    x0 = _start(shape, D)
    L.check(core.lbfgsx_upload(h, L.VEC_X, x0.ctypes.data_as(C.c_void_p)))
    assert s2.minimize_resident(f, n) == want
    got = np.empty(n)
    L.check(core.lbfgsx_download(h, L.VEC_X, got.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(got, x)


# ---------------------------------------------------------------- refusals
def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    f, x0 = A.GridFieldObjective(FR.GL, shape=(20, 25), D=2, scalars=(1.0,)), _start((20, 25), 2)
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, x0.copy())
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, x0.copy())
    with pytest.raises(ValueError, match="shape = \\(20, 25\\), D = 2 does not multiply to n = 999"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(999))
