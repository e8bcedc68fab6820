"""CPU suite: grid stencil objectives compiled at run time (lbfgspp_amd.StencilObjective; lbfgsx_objective_compile_grid_stencil of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import periodic_ref as PR
import stencil_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_stencil_eval", "k_stencil_trial", "k_stencil_b_eval", "k_stencil_b_dg_maxstep_trial")
SHAPES = [(3, 3), (3, 4), (4, 3), (4, 5), (5, 7)]
CASES = [(s, m) for s in SHAPES for m in range(4)]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _instance(shape, dtype):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + 17)
    n = shape[0] * shape[1]
    return rng.standard_normal(n).astype(dtype), (0.5 + rng.random(n)).astype(dtype)


# ---------------------------------------------------------------- the numpy restatement
def _sasym_patch(dt, xs, ws, pos):
    """one patch of SASYM9 in scalar arithmetic of dtype dt, operation for operation"""
    c0, c1 = (dt(v) for v in SR.SASYM_SCALARS)
    m = [dt(v) for v in SR.MULT]
    s0 = dt(dt(dt(ws[0] * xs[0]) + dt(m[1] * dt(ws[1] * xs[1]))) + dt(m[2] * dt(ws[2] * xs[2])))
    s1 = dt(dt(dt(m[3] * dt(ws[3] * xs[3])) + dt(m[4] * dt(ws[4] * xs[4]))) + dt(m[5] * dt(ws[5] * xs[5])))
    s2 = dt(dt(dt(m[6] * dt(ws[6] * xs[6])) + dt(m[7] * dt(ws[7] * xs[7]))) + dt(m[8] * dt(ws[8] * xs[8])))
    q = dt(dt(dt(s0 + s1) + s2) + dt(dt(dt(pos[0]) * c0) + dt(dt(pos[1]) * c1)))
    g = [dt(ws[0] * q)] + [dt(m[k] * dt(ws[k] * q)) for k in range(1, 9)]
    return g, dt(dt(0.5) * dt(q * q))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,mask", CASES)
def test_the_restatement_is_the_scalar_loop_bit_for_bit(shape, mask, dtype):
    """the terms patch by patch with wrapped node indices, the gradient node by node by the lines of include/lbfgsx.h, and
    every existing patch's nine slots used exactly once and no other patch at all"""
    x, p0 = _instance(shape, dtype)
    dt = np.dtype(dtype).type
    rows, cols = shape
    tg, v = SR.sasym9_terms(x, shape, p0)
    ex = SR.exists(shape, mask)
    for r in range(rows):
        for c in range(cols):
            idx = [((r + dr) % rows) * cols + (c + dc) % cols for dr, dc in SR.offsets()]
            g, val = _sasym_patch(dt, [x[k] for k in idx], [p0[k] for k in idx], (r, c))
            assert val.tobytes() == v[r, c].tobytes()
            assert [a.tobytes() for a in g] == [t[r, c].tobytes() for t in tg]
            assert bool(ex[r, c]) == ((c < cols - 2 or bool(mask & 1)) and (r < rows - 2 or bool(mask & 2)))
    for terms in (SR.sasym9_terms(x, shape, p0), SR.plate_terms(x, shape, 0.75)):
        tg, v = terms
        assert v.dtype == dtype and all(a.dtype == dtype and a.shape == tuple(shape) for a in tg)
        grad = SR.stencil_grad(tg, shape, mask)
        loop, used = SR.stencil_grad_scalar(tg, shape, mask)
        assert grad.dtype == dtype and grad.tobytes() == loop.tobytes()
        assert np.array_equal(used, np.broadcast_to(ex[..., None], used.shape).astype(np.int64))


@pytest.mark.parametrize("shape,mask", [(s, m) for s, m in CASES if s in ((4, 5), (5, 7))])
def test_a_centred_difference_of_the_plate_value_agrees_with_its_gradient(shape, mask):
    x, _ = _instance(shape, np.float64)
    n = x.size
    grad = SR.stencil_grad(SR.plate_terms(x, shape, 0.75)[0], shape, mask)
    for k in range(n):
        e = np.zeros(n)
        e[k] = 1e-6
        fd = (SR.value_exact(SR.plate_terms(x + e, shape, 0.75)[1], shape, mask) -
              SR.value_exact(SR.plate_terms(x - e, shape, 0.75)[1], shape, mask)) / 2e-6
        # the energy is quartic: the centred difference errs by h^2 f'''/6 ~ 1e-11 and by rounding ~ 1e-16 f / h ~ 1e-8
        assert abs(fd - grad[k]) <= 1e-6 * (1.0 + abs(grad[k]))


def test_the_per_node_rule_counts_every_node_once():
    """slot (dr, dc) is added by a patch iff (dr == 0 || (!(periodic & 2) && row + 3 == rows)) && (dc == 0 || (!(periodic & 1)
    && col + 3 == cols)), over the existing patches: every node exactly once, at every mask"""
    for shape, mask in CASES:
        rows, cols = shape
        count = np.zeros(shape, np.int64)
        ex = SR.exists(shape, mask)
        for r in range(rows):
            for c in range(cols):
                if not ex[r, c]:
                    continue
                for dr, dc in SR.offsets():
                    if (dr == 0 or (not (mask & 2) and r + 3 == rows)) and (dc == 0 or (not (mask & 1) and c + 3 == cols)):
                        count[(r + dr) % rows, (c + dc) % cols] += 1
        assert np.all(count == 1), (shape, mask)


# ---------------------------------------------------------------- compilation
BODIES = [SR.SASYM9, SR.PLATE]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body", BODIES + [SR.SUB2X2 % PR.PASYM4, SR.ROW3], ids=["sasym9", "plate", "sub2x2", "row3"])
def test_the_bodies_compile_for_both_dtypes_without_scratch(A, body, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.StencilObjective(body, shape=(4, 5))
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert len(info["scratch_by_kernel"]) == 4
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == 9 and core.lbfgsx_objective_form(h) == 13
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_new_kernels(A):
    for body in BODIES:
        for dtype in (np.float64, np.float32):
            src = A.StencilObjective(body, shape=(3, 3)).source(dtype)
            assert src.count(body) == 1
            assert '#include "grid_stencil_kernels.cuh"' in src and "int64_t rows, cols;" in src
            assert "term(const T (&x)[9], T (&g)[9], int64_t i, int64_t row, int64_t col, const int64_t (&j)[9]) const" in src
            assert "struct ObjGridStencil" in src and "static constexpr int K = 9;" in src
            assert "int periodic, pad_;" in src
            for k in KERNELS:
                assert "template __global__ void %s<S, ObjGridStencil>" % k in src
            assert src.count("template __global__") == 4
            assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
            assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)


def test_a_second_compile_is_a_cache_hit_and_the_periodic_grid_form_of_one_text_is_another_entry(A):
    core, _ = A.load()
    # a text that is valid as either: as a patch its g[4..8] stay unset, which this test never runs
    body = "g[0] = x[0]; g[1] = x[1]; g[2] = x[2]; g[3] = x[3]; return x[0] * x[3];\n// cache test of the stencil form"
    sten, grid = A.StencilObjective(body, shape=(3, 3)), A.PeriodicGridObjective(body, shape=(3, 3))
    i_s, i_g = sten.info(), grid.info()
    assert not i_s["cache_hit"] and not i_g["cache_hit"]
    hs, hg = sten.compile(), grid.compile()
    assert hs.value != hg.value and core.lbfgsx_objective_form(hs) == 13 and core.lbfgsx_objective_form(hg) == 10
    # neither the shape nor the mask is part of the key
    again = A.StencilObjective(body, shape=(7, 9), periodic=2).info()
    assert again["cache_hit"] and again["compile_ms"] == i_s["compile_ms"] and again["vgprs"] == i_s["vgprs"]
    assert not A.StencilObjective(body, shape=(3, 3)).info(np.float32)["cache_hit"]


def test_the_mask_of_the_python_class(A):
    assert A.StencilObjective(SR.PLATE, shape=(3, 4)).periodic == 0
    for mask in range(4):
        assert A.StencilObjective(SR.PLATE, shape=(3, 4), periodic=mask).periodic == mask
    assert A.StencilObjective(SR.PLATE, shape=(3, 4), periodic=(True, False)).periodic == 2
    assert A.StencilObjective(SR.PLATE, shape=(3, 4), periodic=(False, True)).periodic == 1
    for bad in (4, -1, 7):
        with pytest.raises(ValueError, match="StencilObjective: periodic = %d: the mask has bit 0" % bad):
            A.StencilObjective(SR.PLATE, shape=(3, 4), periodic=bad)
    with pytest.raises(ValueError, match="periodic must have one flag per axis, \\(rows, cols\\)"):
        A.StencilObjective(SR.PLATE, shape=(3, 4), periodic=(True, True, True))


# ---------------------------------------------------------------- refusals
def test_body_with_inline_assembly_or_nothing_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    fill = "for (int k = 0; k < 9; k++) g[k] = x[0];"
    for body in ("%s volatile(\"\");\n%s\nreturn x[0];" % (word, fill), "%s __%s__(\"\"); return x[0];" % (fill, word)):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.StencilObjective(body, shape=(3, 3)).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    for empty in (b"", None):
        assert core.lbfgsx_objective_compile_grid_stencil(C.byref(h), L.F64, empty, log, len(log)) == L.E_INVALID
        assert not h.value and b"grid stencil objective: empty body" in log.value
        assert core.lbfgsx_objective_source_grid_stencil(L.F64, empty, None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_grid_stencil(C.byref(h), 7, SR.PLATE.encode(), log, len(log)) == L.E_INVALID
    assert b"grid stencil objective: unknown dtype" in log.value


def test_compile_error_comes_back_with_body_relative_lines(A):
    bad = "const T r = x[0];\nfor (int k = 0; k < 9; k++) g[k] = r;\ng[3] = r\nreturn r * r;"  # line 3 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.StencilObjective(bad, shape=(3, 3)).compile()
    assert "StencilObjective" in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)


def test_shapes_and_masks_that_are_refused_by_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for shape in ((2, 6), (6, 2), (0, 0)):
        with pytest.raises(ValueError, match="StencilObjective: shape = \\(%d, %d\\): a 3x3 patch needs at least 3 rows and 3 columns"
                                             % shape):
            A.StencilObjective(SR.PLATE, shape=shape)
    with pytest.raises(ValueError, match="shape must be \\(rows, cols\\)"):
        A.StencilObjective(SR.PLATE, shape=(4, 4, 4))
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="StencilObjective: shape = \\(3, 5\\) does not multiply to n = 16"):
        s.minimize(A.StencilObjective(SR.PLATE, shape=(3, 5), scalars=(1.0,)), np.zeros(16))
    # the C entry points of the solver say the same before a device is needed
    fs, fg = A.StencilObjective(SR.PLATE, shape=(3, 3)), A.PeriodicGridObjective(PR.ALLENCAHN, shape=(3, 3))
    hs, hg = fs.compile(), fg.compile()  # the handles live as long as their objects
    x = np.zeros(12)
    xp = x.ctypes.data_as(C.c_void_p)
    res = L.Result()
    for rows, cols, mask, what in ((2, 6, 3, b"rows = 2, cols = 6"), (6, 2, 3, b"rows = 6, cols = 2"), (-3, -4, 0, b"rows = -3, cols = -4"),
                                   (2 ** 40, 2 ** 40, 1, b"overflows"), (3, 4, 4, b"periodic = 4"), (3, 4, -1, b"periodic = -1")):
        rc = sol.lbfgsx_solver_minimize_grid_stencil(s._h, hs, rows, cols, mask, None, 0, None, xp, None, None, None, C.byref(res))
        assert rc == L.E_INVALID and what in res.msg and b"grid stencil objective: " in res.msg, res.msg
    # lbfgsx_solver_minimize_obj carries no shape; the shaped entry points refuse another form, in both directions
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hs, 12, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"a grid stencil objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_stencil" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_stencil(s._h, hg, 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid stencil objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_periodic(s._h, hs, 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a periodic grid objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_stencil(s._h, fs.compile(np.float32), 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg
    with pytest.raises(ValueError, match="StencilObjective: data\\[0\\] must have 12 elements"):
        s.minimize(A.StencilObjective(SR.SASYM9, shape=(3, 4), data=(np.ones(8),), scalars=SR.SASYM_SCALARS), np.zeros(12))


def test_binding_refusals_name_the_values(A):
    """the bind calls on a context: the context needs a device, so without one the refusals are those of the solver's entry
    points above and this test only checks that no context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64, 24, 3, 0, 0)
    if core.lbfgsx_device_count() <= 0:
        assert rc != 0 and not ctx.value
        return
    assert rc == 0
    try:
        fs, fg = A.StencilObjective(SR.PLATE, shape=(4, 6)), A.PeriodicGridObjective(PR.ALLENCAHN, shape=(4, 6))
        hs, hg = fs.compile(), fg.compile()
        oid = C.c_int(-1)
        for h, args, what in ((hs, (2, 12, 3), "rows = 2, cols = 12"), (hs, (12, 2, 3), "rows = 12, cols = 2"),
                              (hs, (4, 5, 3), "rows = 4, cols = 5 does not multiply to n = 24"),
                              (hs, (2 ** 40, 2 ** 40, 3), "does not multiply to n = 24"), (hs, (4, 6, 4), "periodic = 4"),
                              (hs, (4, 6, -1), "periodic = -1"), (hg, (4, 6, 3), "periodic grid objective, not a grid stencil")):
            assert core.lbfgsx_objective_bind_grid_stencil(ctx, h, *args, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hs, None, None, C.byref(oid)) == L.E_INVALID
        assert "a grid stencil objective is bound with its shape and mask: lbfgsx_objective_bind_grid_stencil" in L.last_error()
        assert core.lbfgsx_objective_bind_grid_periodic(ctx, hs, 4, 6, 3, None, None, C.byref(oid)) == L.E_INVALID
        assert "grid stencil objective, not a periodic grid" in L.last_error()
        assert core.lbfgsx_objective_bind_grid(ctx, hs, 4, 6, None, None, C.byref(oid)) == L.E_INVALID
        assert "grid stencil objective, not a grid" in L.last_error()
        m = C.c_int(-1)
        r, c = C.c_int64(0), C.c_int64(0)
        assert core.lbfgsx_objective_bind_grid_stencil(ctx, hs, 4, 6, 2, None, None, C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == 0 and m.value == 2
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (4, 6)
        assert core.lbfgsx_objective_bind_grid_stencil(ctx, fs.compile(np.float32), 4, 6, 3, None, None, C.byref(oid)) == L.E_INVALID
        assert "the other dtype" in L.last_error()
    finally:
        core.lbfgsx_destroy(ctx)


NEW_CORE = ["lbfgsx_objective_compile_grid_stencil", "lbfgsx_objective_source_grid_stencil", "lbfgsx_objective_bind_grid_stencil"]
NEW_SOLVER = ["lbfgsx_solver_minimize_grid_stencil"]


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
    assert "LBFGSX_FORM_GRID_STENCIL = 13" in text and "grid stencil objectives: 3x3-node terms" in text
    assert "StencilObjective" in A.__all__ and issubclass(A.StencilObjective, A.TermObjective)
    device_h = open(os.path.join(ROOT, "include", "LBFGSpp", "Device.h")).read()
    assert "class StencilObjective : public TermObjective<Scalar>" in device_h


def test_a_translation_unit_with_both_scalar_types_compiles_with_the_host_compiler(tmp_path):
    src = tmp_path / "stencil_tu.cpp"
    src.write_text("#include <Eigen/Core>\n#include <LBFGS.h>\n#include <LBFGSB.h>\n"
                   "using namespace LBFGSpp;\n"
                   "template <class S> int go(const lbfgsx_objective* h)\n{\n"
                   "    typedef Eigen::Matrix<S, Eigen::Dynamic, 1> V;\n"
                   "    StencilObjective<S> f(4, 5, 3, \"return x[4];\");\n    StencilObjective<S> k(h, 4, 5, 0);\n"
                   "    V x = V::Zero(20), lb = V::Constant(20, S(-1)), ub = V::Constant(20, S(1));\n    S fx = 0;\n"
                   "    LBFGSParam<S> p;\n    LBFGSSolver<S> s(p);\n    LBFGSBParam<S> pb;\n    LBFGSBSolver<S> b(pb);\n"
                   "    return s.minimize(f, x, fx) + b.minimize(k, x, fx, lb, ub);\n}\n"
                   "int main() { return go<double>(nullptr) + go<float>(nullptr); }\n")
    cmd = ["g++", "-std=c++17", "-O0", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    cmd = ["g++", "-std=c++17", "-O0", "-fsyntax-only", "-DSTENCIL_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "stencil_probe.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]


def test_generated_wrapper_and_kernel_header_name_no_inline_assembly(A):
    """the text generated around a body and the header it includes hold no inline assembly of their own (the word is spelt in
    pieces so that this file does not hold it either)"""
    word = "as" + "m"
    text = A.StencilObjective(SR.PLATE, shape=(3, 3)).source()
    text += open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "grid_stencil_kernels.cuh")).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text


def test_the_existing_forms_sources_name_none_of_the_new_kernels(A):
    src = A.PeriodicGridObjective(PR.ALLENCAHN, shape=(2, 2)).source()
    assert "stencil" not in src.lower()
