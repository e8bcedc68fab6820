"""CPU suite: volume objectives compiled at run time (lbfgspp_amd.VolumeObjective, lbfgsx_objective_compile_volume of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import volume_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_volume_eval", "k_volume_trial", "k_volume_b_eval", "k_volume_b_dg_maxstep_trial")
SHAPES = [(2, 2, 2), (2, 2, 3), (2, 3, 2), (3, 2, 2), (3, 4, 5), (4, 3, 2)]
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


# ---------------------------------------------------------------- the numpy restatement
def _instance(slabs, rows, cols, dtype):
    rng = np.random.default_rng(10000 * slabs + 100 * rows + cols)
    n = slabs * rows * cols
    return rng.standard_normal(n).astype(dtype), (0.5 + rng.random(n)).astype(dtype)


def _corner_index(slabs, rows, cols, s, r, c):
    return [((s + ds) * rows + r + dr) * cols + c + dc for ds in (0, 1) for dr in (0, 1) for dc in (0, 1)]


@pytest.mark.parametrize("slabs,rows,cols", SHAPES)
def test_the_restatement_sums_every_cell_once(slabs, rows, cols):
    """the exact sum of the restated values against plain loops over the cells in rational arithmetic: every cell once, its
    corners in the order 4*ds + 2*dr + dc"""
    x, p0 = _instance(slabs, rows, cols, np.float64)
    X = [Fraction(float(v)) for v in x]
    P = [Fraction(float(v)) for v in p0]
    c0 = Fraction(0.75)
    k0, k1, k2 = (Fraction(float(np.float64(v))) for v in VR.ASYM_SCALARS)
    exact_ac = exact_as = Fraction(0)
    for s in range(slabs - 1):
        for r in range(rows - 1):
            for c in range(cols - 1):
                idx = _corner_index(slabs, rows, cols, s, r, c)
                u = X[idx[0]] * X[idx[0]] - 1
                exact_ac += Fraction(1, 8) * sum((X[idx[b]] - X[idx[a]]) ** 2 for a, b in EDGES) + c0 * Fraction(1, 4) * u * u
                q = sum(w * P[j] * X[j] for w, j in zip(VR.WEIGHTS, idx)) + s * k0 + r * k1 + c * k2
                exact_as += q * q / 2
    _, v = VR.allencahn3_terms(x, slabs, rows, cols, 0.75)
    assert v.shape == (slabs - 1, rows - 1, cols - 1)
    got = sum(Fraction(float(t)) for t in v.reshape(-1))
    assert abs(got - exact_ac) <= 64 * np.finfo(np.float64).eps * max(1, abs(exact_ac)) * v.size
    _, v = VR.asym8_terms(x, slabs, rows, cols, p0)
    got = sum(Fraction(float(t)) for t in v.reshape(-1))
    assert abs(got - exact_as) <= 64 * np.finfo(np.float64).eps * max(1, abs(exact_as)) * v.size


def _asym8_cell(dt, xs, ws, s, r, c, scalars=VR.ASYM_SCALARS):
    """one cell of ASYM8 in scalar arithmetic of dtype dt, operation for operation"""
    c0, c1, c2 = dt(scalars[0]), dt(scalars[1]), dt(scalars[2])
    s0 = dt(dt(dt(dt(ws[0] * xs[0]) + dt(dt(2) * dt(ws[1] * xs[1]))) + dt(dt(3) * dt(ws[2] * xs[2]))) + dt(dt(5) * dt(ws[3] * xs[3])))
    s1 = dt(dt(dt(dt(dt(7) * dt(ws[4] * xs[4])) + dt(dt(11) * dt(ws[5] * xs[5]))) + dt(dt(13) * dt(ws[6] * xs[6]))) +
            dt(dt(17) * dt(ws[7] * xs[7])))
    q = dt(dt(s0 + s1) + dt(dt(dt(dt(s) * c0) + dt(dt(r) * c1)) + dt(dt(c) * c2)))
    g = [dt(ws[0] * q)] + [dt(dt(w) * dt(ws[j] * q)) for j, w in enumerate(VR.WEIGHTS) if j]
    return g, dt(dt(0.5) * dt(q * q))


def _allencahn3_cell(dt, x, c0):
    a = [dt(x[1] - x[0]), dt(x[3] - x[2]), dt(x[5] - x[4]), dt(x[7] - x[6])]
    b = [dt(x[2] - x[0]), dt(x[3] - x[1]), dt(x[6] - x[4]), dt(x[7] - x[5])]
    e = [dt(x[4] - x[0]), dt(x[5] - x[1]), dt(x[6] - x[2]), dt(x[7] - x[3])]
    u = dt(dt(x[0] * x[0]) - dt(1))
    k = dt(dt(c0) * dt(0.25))
    q = dt(0.25)
    g = [dt(dt(dt(-0.25) * dt(dt(a[0] + b[0]) + e[0])) + dt(dt(dt(4) * k) * dt(u * x[0]))),
         dt(q * dt(dt(a[0] - b[1]) - e[1])), dt(q * dt(dt(b[0] - a[1]) - e[2])), dt(q * dt(dt(a[1] + b[1]) - e[3])),
         dt(q * dt(dt(e[0] - a[2]) - b[2])), dt(q * dt(dt(a[2] + e[1]) - b[3])), dt(q * dt(dt(b[2] + e[2]) - a[3])),
         dt(q * dt(dt(a[3] + b[3]) + e[3]))]

    def squares(d):
        return dt(dt(dt(d[0] * d[0]) + dt(d[1] * d[1])) + dt(dt(d[2] * d[2]) + dt(d[3] * d[3])))
    v = dt(dt(dt(0.125) * dt(dt(squares(a) + squares(b)) + squares(e))) + dt(k * dt(u * u)))
    return g, v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("slabs,rows,cols", SHAPES)
def test_the_restatement_is_the_scalar_loop_bit_for_bit(slabs, rows, cols, dtype):
    x, p0 = _instance(slabs, rows, cols, dtype)
    dt = np.dtype(dtype).type
    n = slabs * rows * cols
    for name in ("asym8", "allencahn3"):
        tg, v = VR.asym8_terms(x, slabs, rows, cols, p0) if name == "asym8" else VR.allencahn3_terms(x, slabs, rows, cols, 0.75)
        assert v.dtype == dtype and len(tg) == 8 and all(a.dtype == dtype for a in tg)
        for s in range(slabs - 1):
            for r in range(rows - 1):
                for c in range(cols - 1):
                    idx = _corner_index(slabs, rows, cols, s, r, c)
                    xs = [x[k] for k in idx]
                    g, val = _asym8_cell(dt, xs, [p0[k] for k in idx], s, r, c) if name == "asym8" else _allencahn3_cell(dt, xs, 0.75)
                    assert val.tobytes() == v[s, r, c].tobytes()
                    assert [a.tobytes() for a in g] == [tg[j][s, r, c].tobytes() for j in range(8)]
        grad = VR.volume_grad(tg, slabs, rows, cols)
        assert grad.dtype == dtype and grad.tobytes() == VR.volume_grad_scalar(tg, slabs, rows, cols).tobytes()
    if dtype == np.float64:  # the gradient is the derivative: central differences of the sum of the values
        for terms in (lambda y: VR.asym8_terms(y, slabs, rows, cols, p0), lambda y: VR.allencahn3_terms(y, slabs, rows, cols, 0.75)):
            grad = VR.volume_grad(terms(x)[0], slabs, rows, cols)
            for j in range(n):
                e = np.zeros(n)
                e[j] = 1e-6
                fd = (terms(x + e)[1].sum() - terms(x - e)[1].sum()) / 2e-6
                assert abs(fd - grad[j]) <= 1e-6 * (1.0 + abs(grad[j]))


def test_the_slab_body_is_the_grid_body_of_the_stacked_rows():
    """SLAB_GRID on (slabs, rows, cols) with p0 zero on the last slab and on every slab's last row against SLAB_GRID_2D's
    restatement on (slabs*rows, cols): what the GPU test asks of the kernels holds for the restatements"""
    import grid_ref as GR
    slabs, rows, cols = 3, 4, 5
    x, p0 = _instance(slabs, rows, cols, np.float64)
    P = p0.reshape(slabs, rows, cols)
    P[-1] = 0
    P[:, -1] = 0
    tg, v = VR.slab_grid_terms(x, slabs, rows, cols, p0)
    x0, x1, x2, x3 = GR.corners(x, slabs * rows, cols)
    s = ((x0 + 2.0 * x1) + 3.0 * x2) + 5.0 * x3
    q = GR.corners(p0, slabs * rows, cols)[0] * s
    g2 = GR.grid_grad([q, 2.0 * q, 3.0 * q, 5.0 * q], slabs * rows, cols)
    assert np.array_equal(VR.volume_grad(tg, slabs, rows, cols), g2) and np.abs(g2).max() > 0
    assert math.fsum(v.reshape(-1)) == math.fsum((0.5 * (q * s)).reshape(-1))  # the grid's extra cells are zeros


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body", [VR.ASYM8, VR.ALLENCAHN3], ids=["asym8", "allencahn3"])
def test_both_bodies_compile_for_both_dtypes_without_scratch(A, body, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.VolumeObjective(body, shape=(3, 4, 5))
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == 8 and core.lbfgsx_objective_form(h) == 9
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_volume_kernels(A):
    for body in (VR.ASYM8, VR.ALLENCAHN3):
        for dtype in (np.float64, np.float32):
            src = A.VolumeObjective(body, shape=(2, 2, 2)).source(dtype)
            assert src.count(body) == 1
            assert '#include "volume_kernels.cuh"' in src and "int64_t slabs, rows, cols;" in src
            assert "term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col) const" in src
            assert "struct ObjVolume" in src and "static constexpr int K = 8;" in src
            for k in KERNELS:
                assert "template __global__ void %s<S, ObjVolume>" % k in src
            assert src.count("template __global__") == 4
            assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
            assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)


def test_grid_and_volume_of_one_body_are_two_cache_entries(A):
    core, _ = A.load()
    # a text that is valid as either: as a volume cell its g[4..7] stay unset, which this test never runs
    body = "g[0] = x[0]; g[1] = x[1]; g[2] = x[2]; g[3] = x[3]; return x[0] * x[3];\n// cache test of the volume form"
    grid, vol = A.GridObjective(body, shape=(2, 2)), A.VolumeObjective(body, shape=(2, 2, 2))
    ig, iv = grid.info(), vol.info()
    assert not ig["cache_hit"] and not iv["cache_hit"]
    hg, hv = grid.compile(), vol.compile()
    assert hg.value != hv.value and core.lbfgsx_objective_form(hg) == 2 and core.lbfgsx_objective_form(hv) == 9
    again = A.VolumeObjective(body, shape=(7, 9, 3)).info()  # the shape is not part of the key
    assert again["cache_hit"] and again["compile_ms"] == iv["compile_ms"] and again["vgprs"] == iv["vgprs"]
    assert A.GridObjective(body, shape=(3, 3)).info()["cache_hit"]
    assert not A.VolumeObjective(body, shape=(2, 2, 2)).info(np.float32)["cache_hit"]


# ---------------------------------------------------------------- refusals
def test_body_with_inline_assembly_or_nothing_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    fill = "for (int k = 0; k < 8; k++) g[k] = x[0];"
    for body in ("%s volatile(\"\");\n%s\nreturn x[0];" % (word, fill), "%s __%s__(\"\"); return x[0];" % (fill, word)):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.VolumeObjective(body, shape=(2, 2, 2)).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    assert core.lbfgsx_objective_compile_volume(C.byref(h), L.F64, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"volume objective: empty body" in log.value
    assert core.lbfgsx_objective_source_volume(L.F64, b"", None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_volume(C.byref(h), 7, VR.ALLENCAHN3.encode(), log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


def test_compile_error_comes_back_with_body_relative_lines(A):
    bad = "const T r = x[0];\nfor (int k = 0; k < 8; k++) g[k] = r;\ng[3] = r\nreturn r * r;"  # line 3 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.VolumeObjective(bad, shape=(2, 2, 2)).compile()
    assert "VolumeObjective" in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)


def test_shapes_that_are_no_volume_are_refused_by_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for shape in ((1, 6, 2), (6, 1, 2), (2, 6, 1), (0, 0, 0)):
        with pytest.raises(ValueError, match="VolumeObjective: shape = \\(%d, %d, %d\\): a volume has at least 2 slabs, 2 rows and "
                                             "2 columns" % shape):
            A.VolumeObjective(VR.ALLENCAHN3, shape=shape)
    with pytest.raises(ValueError, match="shape must be \\(slabs, rows, cols\\)"):
        A.VolumeObjective(VR.ALLENCAHN3, shape=(4, 4))
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="VolumeObjective: shape = \\(2, 3, 5\\) does not multiply to n = 31"):
        s.minimize(A.VolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 5), scalars=(1.0,)), np.zeros(31))
    # the C entry point of the solver says the same before a device is needed
    fv = A.VolumeObjective(VR.ALLENCAHN3, shape=(2, 2, 2))  # the handles live as long as their objects
    h = fv.compile()
    x = np.zeros(12)
    xp = x.ctypes.data_as(C.c_void_p)
    for slabs, rows, cols, what in ((1, 6, 2, b"slabs = 1, rows = 6, cols = 2"), (6, 1, 2, b"slabs = 6, rows = 1, cols = 2"),
                                    (2, 6, 1, b"slabs = 2, rows = 6, cols = 1"), (-2, -3, -2, b"slabs = -2, rows = -3, cols = -2"),
                                    (2 ** 30, 2 ** 30, 2 ** 30, b"overflows"), (2, 2 ** 40, 2 ** 40, b"overflows")):
        res = L.Result()
        rc = sol.lbfgsx_solver_minimize_volume(s._h, h, slabs, rows, cols, None, 0, None, xp, None, None, None, C.byref(res))
        assert rc == L.E_INVALID and what in res.msg and b"volume objective: " in res.msg, res.msg
    # lbfgsx_solver_minimize_obj carries no shape: a volume handle is refused; minimize_volume and minimize_grid refuse another form
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h, 12, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"a volume objective is minimised with its shape: lbfgsx_solver_minimize_volume" in res.msg
    fg = A.GridObjective("g[0] = g[1] = g[2] = g[3] = x[0]; return x[0];", shape=(2, 2))
    rc = sol.lbfgsx_solver_minimize_volume(s._h, fg.compile(), 2, 3, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a volume objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid(s._h, h, 3, 4, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid objective" in res.msg
    # the other dtype
    rc = sol.lbfgsx_solver_minimize_volume(s._h, fv.compile(np.float32), 2, 3, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg
    with pytest.raises(ValueError, match="VolumeObjective: 5 data arrays given, at most 4"):
        A.VolumeObjective(VR.ASYM8, shape=(2, 2, 2), data=[np.ones(8)] * 5)
    with pytest.raises(ValueError, match="VolumeObjective: data\\[0\\] must have 12 elements"):
        s.minimize(A.VolumeObjective(VR.ASYM8, shape=(2, 3, 2), data=(np.ones(8),), scalars=VR.ASYM_SCALARS), np.zeros(12))


def test_binding_refusals_name_the_values(A):
    """lbfgsx_objective_bind_volume, lbfgsx_objective_bind_grid and lbfgsx_objective_bind on a context: the context needs a
    device, so without one the refusals are those of lbfgsx_solver_minimize_volume above and this test only checks that no
    context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64, 24, 3, 0, 0)
    if core.lbfgsx_device_count() <= 0:
        assert rc != 0 and not ctx.value
        return
    assert rc == 0
    try:
        fv = A.VolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 4))  # the handles live as long as their objects
        fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
        hv, hc = fv.compile(), fc.compile()
        oid = C.c_int(-1)
        for h, shape, what in ((hv, (1, 6, 4), "slabs = 1, rows = 6, cols = 4"), (hv, (6, 1, 4), "slabs = 6, rows = 1, cols = 4"),
                               (hv, (6, 4, 1), "slabs = 6, rows = 4, cols = 1"),
                               (hv, (2, 3, 5), "slabs = 2, rows = 3, cols = 5 does not multiply to n = 24"),
                               (hv, (2 ** 30, 2 ** 30, 2 ** 30), "does not multiply to n = 24"),
                               (hc, (2, 3, 4), "chain objective, not a volume")):
            assert core.lbfgsx_objective_bind_volume(ctx, h, *shape, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hv, None, None, C.byref(oid)) == L.E_INVALID
        assert "a volume objective is bound with its shape: lbfgsx_objective_bind_volume" in L.last_error()
        assert core.lbfgsx_objective_bind_grid(ctx, hv, 6, 4, None, None, C.byref(oid)) == L.E_INVALID
        assert "volume objective, not a grid" in L.last_error()
        s, r, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert core.lbfgsx_objective_shape3(ctx, C.byref(s), C.byref(r), C.byref(c)) == L.E_INVALID  # nothing bound yet
        assert core.lbfgsx_objective_bind_volume(ctx, hv, 2, 3, 4, None, None, C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
        assert core.lbfgsx_objective_shape3(ctx, C.byref(s), C.byref(r), C.byref(c)) == 0
        assert (s.value, r.value, c.value) == (2, 3, 4)
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == L.E_INVALID
        assert "no grid objective is bound" in L.last_error()
        hf = fv.compile(np.float32)
        assert core.lbfgsx_objective_bind_volume(ctx, hf, 2, 3, 4, None, None, C.byref(oid)) == L.E_INVALID
        assert "the other dtype" in L.last_error()
    finally:
        core.lbfgsx_destroy(ctx)


NEW_CORE = ["lbfgsx_objective_compile_volume", "lbfgsx_objective_source_volume", "lbfgsx_objective_bind_volume",
            "lbfgsx_objective_shape3"]
NEW_SOLVER = ["lbfgsx_solver_minimize_volume"]


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
    assert "LBFGSX_FORM_VOLUME = 9" in open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    assert "VolumeObjective" in A.__all__ and issubclass(A.VolumeObjective, A.TermObjective)


def test_generated_wrapper_and_kernel_header_name_no_inline_assembly(A):
    """the text generated around a body and the header it includes hold no inline assembly of their own (the word is spelt in
    pieces so that this file does not hold it either)"""
    word = "as" + "m"
    text = A.VolumeObjective(VR.ALLENCAHN3, shape=(2, 2, 2)).source() + open(os.path.join(ROOT, "lbfgspp_amd", "csrc",
                                                                                         "volume_kernels.cuh")).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text
