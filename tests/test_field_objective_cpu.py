"""CPU suite: grid field objectives compiled at run time (lbfgspp_amd.GridFieldObjective; lbfgsx_objective_compile_grid_field of
include/lbfgsx.h; csrc/grid_field_kernels.cuh).  Everything here runs without a GPU: hipRTC compiles for the fixed target
gfx950, and what the code object says about its kernels is read from the code object itself."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import grid_ref as GR
import periodic_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_gfield_eval", "k_gfield_trial", "k_gfield_b_eval", "k_gfield_b_dg_maxstep_trial")
SHAPES = [(2, 2), (2, 3), (3, 2), (3, 5), (5, 3)]
CASES = [(s, m, D) for s in SHAPES for m in range(4) for D in (1, 2, 3)]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _instance(shape, D, dtype):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + D)
    n = shape[0] * shape[1] * D
    return rng.standard_normal(n).astype(dtype), (0.5 + rng.random(n)).astype(dtype)


def _terms(name, x, shape, D, p0):
    return FR.fasym_terms(x, shape, D, p0) if name == "fasym" else FR.gl_terms(x, shape, D, 0.75)


# ---------------------------------------------------------------- the numpy restatement
def _fasym_cell(dt, D, xs, ws, pos):
    """one cell of FASYM in scalar arithmetic of dtype dt, operation for operation; xs, ws slot-major"""
    c0, c1 = (dt(v) for v in FR.FASYM_SCALARS)
    w, s = [], dt(0)
    for k in range(4):
        for d in range(D):
            w.append(dt(ws[k * D + d] * dt(1 + 2 * k + 7 * d)))
            s = dt(s + dt(w[-1] * xs[k * D + d]))
    q = dt(s + dt(dt(dt(pos[0]) * c0) + dt(dt(pos[1]) * c1)))
    return [dt(wm * q) for wm in w], dt(dt(0.5) * dt(q * q))


def _gl_cell(dt, D, xs, c0):
    ss = dt(0)
    for d in range(D):
        ss = dt(ss + dt(xs[d] * xs[d]))
    u = dt(ss - dt(1))
    k = dt(dt(c0) * dt(0.25))
    g, v = [None] * (4 * D), dt(0)
    for d in range(D):
        a, b = dt(xs[D + d] - xs[d]), dt(xs[2 * D + d] - xs[d])
        e, h = dt(xs[3 * D + d] - xs[2 * D + d]), dt(xs[3 * D + d] - xs[D + d])
        g[d] = dt(dt(dt(-0.5) * dt(a + b)) + dt(dt(dt(4) * k) * dt(u * xs[d])))
        g[D + d] = dt(dt(0.5) * dt(a - h))
        g[2 * D + d] = dt(dt(0.5) * dt(b - e))
        g[3 * D + d] = dt(dt(0.5) * dt(e + h))
        v = dt(v + dt(dt(dt(a * a) + dt(b * b)) + dt(dt(e * e) + dt(h * h))))
    return g, dt(dt(dt(0.25) * v) + dt(k * dt(u * u)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,mask,D", CASES)
def test_the_restatement_is_the_scalar_loop_bit_for_bit(shape, mask, D, dtype):
    """the terms cell by cell with wrapped node indices j[k] and flat coordinates j[k]*D + d, the gradient node by node and
    unknown by unknown by the rule of include/lbfgsx.h, every existing cell counted once per slot and no other cell at all"""
    x, p0 = _instance(shape, D, dtype)
    dt = np.dtype(dtype).type
    rows, cols = shape
    ex = FR.exists(shape, mask)
    fa, gl = _terms("fasym", x, shape, D, p0), _terms("gl", x, shape, D, p0)
    for r, c in itertools.product(range(rows), range(cols)):
        j = [((r + dr) % rows) * cols + (c + dc) % cols for dr, dc in PR.offsets(2)]
        flat = [j[k] * D + d for k in range(4) for d in range(D)]
        for (tg, v), (g, val) in ((fa, _fasym_cell(dt, D, [x[i] for i in flat], [p0[i] for i in flat], (r, c))),
                                  (gl, _gl_cell(dt, D, [x[i] for i in flat], 0.75))):
            assert val.tobytes() == v[r, c].tobytes()
            assert [a.tobytes() for a in g] == [t[r, c].tobytes() for t in tg]
        assert bool(ex[r, c]) == ((c < cols - 1 or bool(mask & 1)) and (r < rows - 1 or bool(mask & 2)))
    for tg, v in (fa, gl):
        assert v.dtype == dtype and len(tg) == 4 * D and all(a.dtype == dtype and a.shape == tuple(shape) for a in tg)
        grad = FR.field_grad(tg, shape, D, mask)
        loop, used = FR.field_grad_scalar(tg, shape, D, mask)
        assert grad.dtype == dtype and grad.tobytes() == loop.tobytes()
        assert np.array_equal(used, np.broadcast_to(ex[..., None], used.shape).astype(np.int64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_at_one_unknown_per_node_the_restatement_is_the_periodic_grids(dtype):
    for shape in SHAPES:
        x, p0 = _instance(shape, 1, dtype)
        for mask in range(4):
            tg, v = FR.gl_terms(x, shape, 1, 0.75)
            assert FR.field_grad(tg, shape, 1, mask).tobytes() == PR.periodic_grad(tg, shape, mask).tobytes()
            assert FR.values(v, shape, mask).tobytes() == PR.values(v, shape, mask).tobytes()
            # the same energy as the periodic form's Allen-Cahn text, term by term (the value's sum starts from 0 + here)
            tp, vp = PR.allencahn_terms(x, shape, 0.75)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(tg, tp)) and np.array_equal(v, vp)


@pytest.mark.parametrize("mask", range(4))
@pytest.mark.parametrize("D", [1, 2, 3])
def test_the_gradient_is_the_derivative_of_the_sum_of_the_existing_cells(mask, D):
    shape = (3, 5)
    x, p0 = _instance(shape, D, np.float64)
    for name in ("fasym", "gl"):
        grad = FR.field_grad(_terms(name, x, shape, D, p0)[0], shape, D, mask)
        for k in range(x.size):
            e = np.zeros(x.size)
            e[k] = 1e-6
            fd = (FR.value_exact(_terms(name, x + e, shape, D, p0)[1], shape, mask) -
                  FR.value_exact(_terms(name, x - e, shape, D, p0)[1], shape, mask)) / 2e-6
            assert abs(fd - grad[k]) <= 1e-6 * (1.0 + abs(grad[k]))


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("shape", [(3, 5), (5, 2)])
def test_on_a_torus_rolling_x_by_whole_nodes_rolls_the_gradient(shape, D):
    x, p0 = _instance(shape, D, np.float64)
    full = tuple(shape) + (D,)
    g = FR.field_grad(FR.fasym_terms(x, shape, D, p0, (0.0, 0.0))[0], shape, D, 3).reshape(full)
    for shift in itertools.product(range(shape[0]), range(shape[1])):
        xr, pr = (np.roll(a.reshape(full), shift, (0, 1)).reshape(-1) for a in (x, p0))
        gr = FR.field_grad(FR.fasym_terms(xr, shape, D, pr, (0.0, 0.0))[0], shape, D, 3).reshape(full)
        assert gr.tobytes() == np.roll(g, shift, (0, 1)).tobytes()


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("body", [FR.FASYM, FR.GL], ids=["fasym", "gl"])
def test_both_bodies_compile_for_every_D_and_dtype_without_scratch(A, body, D, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.GridFieldObjective(body, shape=(4, 5), D=D)
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_form(h) == 12 and core.lbfgsx_objective_K(h) == 4 and core.lbfgsx_objective_D(h) == D
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_new_kernels(A):
    for body, D, dtype in itertools.product((FR.FASYM, FR.GL), (1, 2, 3), (np.float64, np.float32)):
        src = A.GridFieldObjective(body, shape=(2, 2), D=D).source(dtype)
        assert src.count(body) == 1
        assert '#include "grid_field_kernels.cuh"' in src and "struct ObjGridField" in src
        assert "static constexpr int D = %d;" % D in src and "static constexpr int K = 4;" in src
        assert "int64_t rows, cols;" in src and "int periodic, pad_;" in src
        assert ("term(const T (&x)[4 * D], T (&g)[4 * D], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const") in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjGridField>" % k in src
        assert src.count("template __global__") == 4
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)


def test_the_open_and_periodic_forms_sources_name_nothing_of_the_new_form(A):
    for src in (A.GridObjective(GR.ALLENCAHN, shape=(2, 2)).source(), A.PeriodicGridObjective(PR.ALLENCAHN, shape=(2, 2)).source()):
        assert "gfield" not in src and "grid_field" not in src and "ObjGridField" not in src and "constexpr int D" not in src


def test_D_is_part_of_the_cache_key_and_shape_and_mask_are_not(A):
    core, _ = A.load()
    body = "for (int m = 0; m < 4 * D; m++) g[m] = x[m]; return x[0] * x[3 * D];\n// cache test of the grid field form"
    f2, f3 = A.GridFieldObjective(body, shape=(2, 2), D=2), A.GridFieldObjective(body, shape=(2, 2), D=3)
    i2, i3 = f2.info(), f3.info()
    assert not i2["cache_hit"] and not i3["cache_hit"]
    h2, h3 = f2.compile(), f3.compile()
    assert h2.value != h3.value and core.lbfgsx_objective_D(h2) == 2 and core.lbfgsx_objective_D(h3) == 3
    again = A.GridFieldObjective(body, shape=(7, 9), D=3, periodic=(True, False)).info()
    assert again["cache_hit"] and again["compile_ms"] == i3["compile_ms"] and again["vgprs"] == i3["vgprs"]
    assert A.GridFieldObjective(body, shape=(3, 4), D=2, periodic=(True, True)).info()["cache_hit"]
    assert not A.GridFieldObjective(body, shape=(2, 2), D=2).info(np.float32)["cache_hit"]
    # one text at D = 1 as a field and as a periodic grid objective: two entries, in either order
    one = "g[0] = x[0]; g[1] = x[1]; g[2] = x[2]; g[3] = x[3]; return x[0] * x[3];\n// cache test of the grid field form at D = 1"
    assert not A.GridFieldObjective(one, shape=(2, 2), D=1).info()["cache_hit"]
    assert not A.PeriodicGridObjective(one, shape=(2, 2)).info()["cache_hit"]
    assert A.GridFieldObjective(one, shape=(5, 2), D=1, periodic=(True, True)).info()["cache_hit"]


def test_one_text_compiles_as_a_field_at_D_1_and_as_a_periodic_grid_objective(A):
    core, _ = A.load()
    field, per = A.GridFieldObjective(PR.PASYM4, shape=(2, 2), D=1), A.PeriodicGridObjective(PR.PASYM4, shape=(2, 2))
    assert field.info()["scratch_bytes"] == 0 and per.info()["scratch_bytes"] == 0
    assert core.lbfgsx_objective_form(field.compile()) == 12 and core.lbfgsx_objective_form(per.compile()) == 10
    assert field.compile().value != per.compile().value


def test_the_mask_and_D_of_the_python_class(A):
    assert A.GridFieldObjective(FR.GL, shape=(2, 3), D=2).periodic == 0  # open by default
    assert A.GridFieldObjective(FR.GL, shape=(2, 3), D=2, periodic=(True, False)).periodic == 2
    assert A.GridFieldObjective(FR.GL, shape=(2, 3), D=2, periodic=(False, True)).periodic == 1
    f = A.GridFieldObjective(FR.GL, shape=(2, 3), D=3, periodic=(True, True))
    assert (f.periodic, f.D, f.K, f.shape) == (3, 3, 4, (2, 3))
    for bad in ((True,), (True, True, True), True):
        with pytest.raises(ValueError, match="GridFieldObjective: periodic must have one flag per axis, \\(rows, cols\\)"):
            A.GridFieldObjective(FR.GL, shape=(2, 3), D=2, periodic=bad)
    with pytest.raises(ValueError, match="GridFieldObjective: periodic = .*: a flag is True or False"):
        A.GridFieldObjective(FR.GL, shape=(2, 3), D=2, periodic=(True, 2))


# ---------------------------------------------------------------- refusals
def test_D_outside_1_to_3_is_refused_with_its_value(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for D in (0, 4, -1, 2.0, True):
        with pytest.raises(ValueError, match="GridFieldObjective: D = .* is not supported: a node has D = 1, 2 or 3 unknowns"):
            A.GridFieldObjective(FR.GL, shape=(2, 3), D=D)
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    for D in (0, 4):
        want = ("grid field objective: D = %d is not supported: a node has D = 1, 2 or 3 unknowns" % D).encode()
        assert core.lbfgsx_objective_compile_grid_field(C.byref(h), L.F64, D, FR.GL.encode(), log, len(log)) == L.E_INVALID
        assert not h.value and want in log.value
        assert core.lbfgsx_objective_source_grid_field(L.F64, D, FR.GL.encode(), None, 0) == L.E_INVALID
        assert want.decode() in L.last_error()


def test_body_with_inline_assembly_or_nothing_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    fill = "for (int k = 0; k < 4 * D; k++) g[k] = x[0];"
    for body in ("%s volatile(\"\");\n%s\nreturn x[0];" % (word, fill), "%s __%s__(\"\"); return x[0];" % (fill, word)):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.GridFieldObjective(body, shape=(2, 2), D=2).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    for empty in (b"", None):
        assert core.lbfgsx_objective_compile_grid_field(C.byref(h), L.F64, 2, empty, log, len(log)) == L.E_INVALID
        assert not h.value and b"grid field objective: empty body" in log.value
        assert core.lbfgsx_objective_source_grid_field(L.F64, 2, empty, None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_grid_field(C.byref(h), 7, 2, FR.GL.encode(), log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


def test_compile_error_comes_back_with_body_relative_lines(A):
    bad = "const T r = x[0];\nfor (int k = 0; k < 4 * D; k++) g[k] = r;\ng[3] = r\nreturn r * r;"  # line 3 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.GridFieldObjective(bad, shape=(2, 2), D=2).compile()
    assert "GridFieldObjective" in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)


def test_shapes_and_masks_that_are_refused_by_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for shape in ((1, 6), (6, 1), (0, 0)):
        with pytest.raises(ValueError, match="GridFieldObjective: shape = \\(%d, %d\\): a grid has at least 2 rows and 2 columns" % shape):
            A.GridFieldObjective(FR.GL, shape=shape, D=2)
    with pytest.raises(ValueError, match="shape must be \\(rows, cols\\)"):
        A.GridFieldObjective(FR.GL, shape=(4, 4, 4), D=2)
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="GridFieldObjective: shape = \\(3, 5\\), D = 2 does not multiply to n = 15"):
        s.minimize(A.GridFieldObjective(FR.GL, shape=(3, 5), D=2, scalars=(1.0,)), np.zeros(15))
    with pytest.raises(ValueError, match="GridFieldObjective: data\\[0\\] must have 24 elements"):
        s.minimize(A.GridFieldObjective(FR.FASYM, shape=(3, 4), D=2, data=(np.ones(12),), scalars=FR.FASYM_SCALARS), np.zeros(24))
    # the C entry point of the solver says the same before a device is needed
    f2 = A.GridFieldObjective(FR.GL, shape=(2, 2), D=2)
    h2 = f2.compile()  # the handle lives as long as its object
    x = np.zeros(24)
    xp = x.ctypes.data_as(C.c_void_p)
    res = L.Result()
    for rows, cols, mask, what in ((1, 12, 3, b"rows = 1, cols = 12, D = 2"), (12, 1, 3, b"rows = 12, cols = 1, D = 2"),
                                   (-3, -4, 0, b"rows = -3, cols = -4, D = 2"), (2 ** 31, 2 ** 31, 1, b"rows*cols*D overflows"),
                                   (2 ** 40, 2 ** 40, 1, b"overflows"), (3, 4, 4, b"periodic = 4"), (3, 4, -1, b"periodic = -1")):
        rc = sol.lbfgsx_solver_minimize_grid_field(s._h, h2, rows, cols, mask, None, 0, None, xp, None, None, None, C.byref(res))
        assert rc == L.E_INVALID and what in res.msg and b"grid field objective: " in res.msg, res.msg
    # a wrong handle form in each direction
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h2, 24, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"a grid field objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_field" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_periodic(s._h, h2, 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a periodic grid objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid(s._h, h2, 3, 4, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid objective" in res.msg
    per = A.PeriodicGridObjective(PR.ALLENCAHN, shape=(2, 2))
    rc = sol.lbfgsx_solver_minimize_grid_field(s._h, per.compile(), 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid field objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_field(s._h, f2.compile(np.float32), 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg


def test_binding_refusals_name_the_values(A):
    """the bind call on a context: the context needs a device, so without one the refusals are those of the solver's entry
    point above and this test only checks that no context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64, 48, 3, 0, 0)
    if core.lbfgsx_device_count() <= 0:
        assert rc != 0 and not ctx.value
        return
    assert rc == 0
    try:
        ff, fp = A.GridFieldObjective(FR.GL, shape=(4, 6), D=2), A.PeriodicGridObjective(PR.ALLENCAHN, shape=(4, 6))
        hf, hp = ff.compile(), fp.compile()
        oid = C.c_int(-1)
        for h, args, what in ((hf, (1, 24, 3), "rows = 1, cols = 24, D = 2"), (hf, (24, 1, 3), "rows = 24, cols = 1, D = 2"),
                              (hf, (4, 5, 3), "rows = 4, cols = 5, D = 2 does not multiply to n = 48"),
                              (hf, (8, 6, 3), "rows = 8, cols = 6, D = 2 does not multiply to n = 48"),
                              (hf, (2 ** 40, 2 ** 40, 3), "does not multiply to n = 48"), (hf, (4, 6, 4), "periodic = 4"),
                              (hf, (4, 6, -1), "periodic = -1"), (hp, (4, 6, 3), "periodic grid objective, not a grid field")):
            assert core.lbfgsx_objective_bind_grid_field(ctx, h, *args, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hf, None, None, C.byref(oid)) == L.E_INVALID
        assert "a grid field objective is bound with its shape, mask and D: lbfgsx_objective_bind_grid_field" in L.last_error()
        assert core.lbfgsx_objective_bind_grid_periodic(ctx, hf, 4, 6, 3, None, None, C.byref(oid)) == L.E_INVALID
        assert "grid field objective, not a periodic grid" in L.last_error()
        assert core.lbfgsx_objective_bind_grid(ctx, hf, 4, 6, None, None, C.byref(oid)) == L.E_INVALID
        assert "grid field objective, not a grid" in L.last_error()
        m, r, c = C.c_int(-1), C.c_int64(0), C.c_int64(0)
        assert core.lbfgsx_objective_bind_grid_field(ctx, hf, 4, 6, 2, None, None, C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == 0 and m.value == 2
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (4, 6)
        assert core.lbfgsx_objective_D(hf) == 2
        assert core.lbfgsx_objective_bind_grid_field(ctx, ff.compile(np.float32), 4, 6, 3, None, None, C.byref(oid)) == L.E_INVALID
        assert "the other dtype" in L.last_error()
    finally:
        core.lbfgsx_destroy(ctx)


NEW_CORE = ["lbfgsx_objective_compile_grid_field", "lbfgsx_objective_source_grid_field", "lbfgsx_objective_bind_grid_field",
            "lbfgsx_objective_D"]
NEW_SOLVER = ["lbfgsx_solver_minimize_grid_field"]


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
    text = open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    assert "LBFGSX_FORM_GRID_FIELD = 12" in text and "LBFGSX_FORM_GRID_PERIODIC = 10" in text
    assert "GridFieldObjective" in A.__all__ and issubclass(A.GridFieldObjective, A.TermObjective)
    device_h = open(os.path.join(ROOT, "include", "LBFGSpp", "Device.h")).read()
    assert "class GridFieldObjective : public TermObjective<Scalar>" in device_h


def test_the_new_kernel_header_names_no_inline_assembly(A):
    word = "as" + "m"
    text = A.GridFieldObjective(FR.GL, shape=(2, 2), D=3).source()
    text += open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "grid_field_kernels.cuh")).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text
