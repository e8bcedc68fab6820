"""CPU suite: grid objectives compiled at run time (lbfgspp_amd.GridObjective, lbfgsx_objective_compile_grid of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import grid_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_grid_eval", "k_grid_trial", "k_grid_b_eval", "k_grid_b_dg_maxstep_trial")
SHAPES = [(2, 2), (2, 3), (3, 2), (3, 5), (5, 4), (4, 7)]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


# ---------------------------------------------------------------- the numpy restatement
def _instance(rows, cols, dtype):
    rng = np.random.default_rng(1000 * rows + cols)
    n = rows * cols
    return rng.standard_normal(n).astype(dtype), (0.5 + rng.random(n)).astype(dtype)


def _allencahn_cell_exact(x0, x1, x2, x3, c0):
    a, b, e, h, u = x1 - x0, x2 - x0, x3 - x2, x3 - x1, x0 * x0 - 1
    return Fraction(1, 4) * (a * a + b * b + e * e + h * h) + c0 * Fraction(1, 4) * u * u


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_restatement_sums_every_cell_once(rows, cols):
    """the exact sum of the restated values against plain loops over the cells in rational arithmetic: every cell once, its
    corners in the order (r,c), (r,c+1), (r+1,c), (r+1,c+1)"""
    x, p0 = _instance(rows, cols, np.float64)
    X = [[Fraction(float(x[r * cols + c])) for c in range(cols)] for r in range(rows)]
    P = [[Fraction(float(p0[r * cols + c])) for c in range(cols)] for r in range(rows)]
    c0 = Fraction(0.75)
    k0, k1 = (Fraction(float(np.float64(v))) for v in GR.ASYM_SCALARS)
    exact_ac = exact_as = Fraction(0)
    for r in range(rows - 1):
        for c in range(cols - 1):
            exact_ac += _allencahn_cell_exact(X[r][c], X[r][c + 1], X[r + 1][c], X[r + 1][c + 1], c0)
            q = (P[r][c] * X[r][c] + 2 * P[r][c + 1] * X[r][c + 1] + 3 * P[r + 1][c] * X[r + 1][c] +
                 5 * P[r + 1][c + 1] * X[r + 1][c + 1] + r * k0 + c * k1)
            exact_as += q * q / 2
    _, v = GR.allencahn_terms(x, rows, cols, 0.75)
    assert v.shape == (rows - 1, cols - 1)
    got = sum(Fraction(float(t)) for t in v.reshape(-1))
    assert abs(got - exact_ac) <= 64 * np.finfo(np.float64).eps * max(1, abs(exact_ac)) * v.size
    _, v = GR.asym4_terms(x, rows, cols, p0)
    got = sum(Fraction(float(t)) for t in v.reshape(-1))
    assert abs(got - exact_as) <= 64 * np.finfo(np.float64).eps * max(1, abs(exact_as)) * v.size


def _asym4_cell(dt, xs, ws, r, c, scalars=GR.ASYM_SCALARS):
    """one cell of ASYM4 in scalar arithmetic of dtype dt, operation for operation"""
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    s = dt(dt(dt(dt(ws[0] * xs[0]) + dt(dt(2) * dt(ws[1] * xs[1]))) + dt(dt(3) * dt(ws[2] * xs[2]))) + dt(dt(5) * dt(ws[3] * xs[3])))
    q = dt(s + dt(dt(dt(r) * c0) + dt(dt(c) * c1)))
    g = [dt(ws[0] * q), dt(dt(2) * dt(ws[1] * q)), dt(dt(3) * dt(ws[2] * q)), dt(dt(5) * dt(ws[3] * q))]
    return g, dt(dt(0.5) * dt(q * q))


def _allencahn_cell(dt, xs, c0):
    a, b, e, h = dt(xs[1] - xs[0]), dt(xs[2] - xs[0]), dt(xs[3] - xs[2]), dt(xs[3] - xs[1])
    u = dt(dt(xs[0] * xs[0]) - dt(1))
    k = dt(dt(c0) * dt(0.25))
    g = [dt(dt(dt(-0.5) * dt(a + b)) + dt(dt(dt(4) * k) * dt(u * xs[0]))), dt(dt(0.5) * dt(a - h)), dt(dt(0.5) * dt(b - e)),
         dt(dt(0.5) * dt(e + h))]
    v = dt(dt(dt(0.25) * dt(dt(dt(a * a) + dt(b * b)) + dt(dt(e * e) + dt(h * h)))) + dt(k * dt(u * u)))
    return g, v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_restatement_is_the_scalar_loop_bit_for_bit(rows, cols, dtype):
    x, p0 = _instance(rows, cols, dtype)
    dt = np.dtype(dtype).type
    for name in ("asym4", "allencahn"):
        tg, v = GR.asym4_terms(x, rows, cols, p0) if name == "asym4" else GR.allencahn_terms(x, rows, cols, 0.75)
        assert v.dtype == dtype and all(a.dtype == dtype for a in tg)
        for r in range(rows - 1):
            for c in range(cols - 1):
                idx = [r * cols + c, r * cols + c + 1, (r + 1) * cols + c, (r + 1) * cols + c + 1]
                xs = [x[k] for k in idx]
                g, val = _asym4_cell(dt, xs, [p0[k] for k in idx], r, c) if name == "asym4" else _allencahn_cell(dt, xs, 0.75)
                assert val.tobytes() == v[r, c].tobytes()
                assert [a.tobytes() for a in g] == [tg[j][r, c].tobytes() for j in range(4)]
        grad = GR.grid_grad(tg, rows, cols)
        assert grad.dtype == dtype and grad.tobytes() == GR.grid_grad_scalar(tg, rows, cols).tobytes()
    if dtype == np.float64:  # the gradient is the derivative: central differences of the sum of the values
        grad = GR.grid_grad(GR.asym4_terms(x, rows, cols, p0)[0], rows, cols)
        for j in range(rows * cols):
            e = np.zeros(rows * cols)
            e[j] = 1e-6
            fd = (GR.asym4_terms(x + e, rows, cols, p0)[1].sum() - GR.asym4_terms(x - e, rows, cols, p0)[1].sum()) / 2e-6
            assert abs(fd - grad[j]) <= 1e-6 * (1.0 + abs(grad[j]))


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body", [GR.ASYM4, GR.ALLENCAHN], ids=["asym4", "allencahn"])
def test_both_bodies_compile_for_both_dtypes_without_scratch(A, body, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.GridObjective(body, shape=(3, 5))
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == 4 and core.lbfgsx_objective_form(h) == 2
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_grid_kernels(A):
    for body in (GR.ASYM4, GR.ALLENCAHN):
        for dtype in (np.float64, np.float32):
            src = A.GridObjective(body, shape=(2, 2)).source(dtype)
            assert src.count(body) == 1
            assert '#include "grid_kernels.cuh"' in src and "int64_t rows, cols;" in src
            assert "term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col)" in src
            for k in KERNELS:
                assert "template __global__ void %s<S, ObjGrid>" % k in src
            assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
            assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)


def test_chain_and_grid_of_one_body_are_two_cache_entries(A):
    core, _ = A.load()
    # a text that is valid as either: as a grid cell its g[2] and g[3] stay unset, which this test never runs
    body = "g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];\n// cache test of the grid form"
    chain, grid = A.ChainObjective(body, K=2), A.GridObjective(body, shape=(2, 2))
    ic, ig = chain.info(), grid.info()
    assert not ic["cache_hit"] and not ig["cache_hit"]
    hc, hg = chain.compile(), grid.compile()
    assert hc.value != hg.value and core.lbfgsx_objective_form(hc) == 1 and core.lbfgsx_objective_form(hg) == 2
    again = A.GridObjective(body, shape=(7, 9)).info()  # the shape is not part of the key
    assert again["cache_hit"] and again["compile_ms"] == ig["compile_ms"] and again["vgprs"] == ig["vgprs"]
    assert A.ChainObjective(body, K=2).info()["cache_hit"]
    assert not A.GridObjective(body, shape=(2, 2)).info(np.float32)["cache_hit"]


# ---------------------------------------------------------------- refusals
def test_body_with_inline_assembly_or_nothing_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    for body in ("%s volatile(\"\");\ng[0] = g[1] = g[2] = g[3] = x[0];\nreturn x[0];" % word,
                 "g[0] = g[1] = g[2] = g[3] = x[0]; __%s__(\"\"); return x[0];" % word):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.GridObjective(body, shape=(2, 2)).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    assert core.lbfgsx_objective_compile_grid(C.byref(h), L.F64, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"grid objective: empty body" in log.value
    assert core.lbfgsx_objective_source_grid(L.F64, b"", None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_grid(C.byref(h), 7, GR.ALLENCAHN.encode(), log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


def test_compile_error_comes_back_with_body_relative_lines(A):
    bad = "const T r = x[0];\ng[0] = g[1] = g[2] = r;\ng[3] = r\nreturn r * r;"  # line 3 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.GridObjective(bad, shape=(2, 2)).compile()
    assert "GridObjective" in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)


def test_shapes_that_are_no_grid_are_refused_by_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for shape in ((1, 6), (6, 1), (0, 0)):
        with pytest.raises(ValueError, match="GridObjective: shape = \\(%d, %d\\): a grid has at least 2 rows and 2 columns" % shape):
            A.GridObjective(GR.ALLENCAHN, shape=shape)
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="GridObjective: shape = \\(3, 5\\) does not multiply to n = 16"):
        s.minimize(A.GridObjective(GR.ALLENCAHN, shape=(3, 5), scalars=(1.0,)), np.zeros(16))
    # the C entry point of the solver says the same before a device is needed
    fg = A.GridObjective(GR.ALLENCAHN, shape=(2, 2))  # the handles live as long as their objects
    h = fg.compile()
    x = np.zeros(6)
    for rows, cols, what in ((1, 6, b"rows = 1, cols = 6"), (6, 1, b"rows = 6, cols = 1"), (-2, -3, b"rows = -2, cols = -3"),
                             (2 ** 40, 2 ** 40, b"overflows")):
        res = L.Result()
        rc = sol.lbfgsx_solver_minimize_grid(s._h, h, rows, cols, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None,
                                             C.byref(res))
        assert rc == L.E_INVALID and what in res.msg, res.msg
    # lbfgsx_solver_minimize_obj carries no shape: a grid handle is refused; minimize_grid refuses another form
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h, 6, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"lbfgsx_solver_minimize_grid" in res.msg
    fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
    hc = fc.compile()
    rc = sol.lbfgsx_solver_minimize_grid(s._h, hc, 2, 3, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid objective" in res.msg
    # the other dtype
    rc = sol.lbfgsx_solver_minimize_grid(s._h, fg.compile(np.float32), 2, 3, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None,
                                         None, C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg
    with pytest.raises(ValueError, match="GridObjective: 5 data arrays given, at most 4"):
        A.GridObjective(GR.ASYM4, shape=(2, 2), data=[np.ones(4)] * 5)
    with pytest.raises(ValueError, match="GridObjective: data\\[0\\] must have 6 elements"):
        s.minimize(A.GridObjective(GR.ASYM4, shape=(2, 3), data=(np.ones(4),), scalars=GR.ASYM_SCALARS), np.zeros(6))


def _no_gpu(core):
    return core.lbfgsx_device_count() <= 0


def test_binding_refusals_name_the_values(A):
    """lbfgsx_objective_bind_grid and lbfgsx_objective_bind on a context: the context needs a device, so without one the
    refusals are those of lbfgsx_solver_minimize_grid above and this test only checks that no context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64, 12, 3, 0, 0)
    if _no_gpu(core):
        assert rc != 0 and not ctx.value
        return
    assert rc == 0
    try:
        fg = A.GridObjective(GR.ALLENCAHN, shape=(3, 4))  # the handles live as long as their objects
        fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
        hg, hc = fg.compile(), fc.compile()
        oid = C.c_int(-1)
        for h, rows, cols, what in ((hg, 1, 12, "rows = 1, cols = 12"), (hg, 12, 1, "rows = 12, cols = 1"),
                                    (hg, 3, 5, "rows = 3, cols = 5 does not multiply to n = 12"),
                                    (hg, 2 ** 40, 2 ** 40, "does not multiply to n = 12"), (hc, 3, 4, "chain objective, not a grid")):
            assert core.lbfgsx_objective_bind_grid(ctx, h, rows, cols, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hg, None, None, C.byref(oid)) == L.E_INVALID
        assert "a grid objective is bound with its shape: lbfgsx_objective_bind_grid" in L.last_error()
        r, c = C.c_int64(0), C.c_int64(0)
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == L.E_INVALID  # nothing bound yet
        assert core.lbfgsx_objective_bind_grid(ctx, hg, 3, 4, None, None, C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (3, 4)
        hf = fg.compile(np.float32)
        assert core.lbfgsx_objective_bind_grid(ctx, hf, 3, 4, None, None, C.byref(oid)) == L.E_INVALID
        assert "the other dtype" in L.last_error()
    finally:
        core.lbfgsx_destroy(ctx)


NEW_CORE = ["lbfgsx_objective_compile_grid", "lbfgsx_objective_source_grid", "lbfgsx_objective_bind_grid", "lbfgsx_objective_shape"]
NEW_SOLVER = ["lbfgsx_solver_minimize_grid"]


def test_new_symbols_are_exported_and_declared(A):
    listed = open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "export.map")).read()

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lbfgspp_amd", lib)], stdout=subprocess.PIPE,
                             text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    for names, lib, header in ((NEW_CORE, "liblbfgsx.so", "lbfgsx.h"), (NEW_SOLVER, "liblbfgsx_solver.so", "lbfgsx_solver.h")):
        have, text = exported(lib), open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert name in have, "%s does not export %s" % (lib, name)
            assert name + ";" in listed, "export.map does not list %s" % name
            assert name + "(" in text, "%s does not declare %s" % (header, name)
    assert "LBFGSX_FORM_GRID = 2" in open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    assert "GridObjective" in A.__all__


def test_generated_wrapper_and_kernel_header_name_no_inline_assembly(A):
    """the text generated around a body and the header it includes hold no inline assembly of their own (the word is spelt in
    pieces so that this file does not hold it either)"""
    word = "as" + "m"
    text = A.GridObjective(GR.ALLENCAHN, shape=(2, 2)).source() + open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "grid_kernels.cuh")).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text
