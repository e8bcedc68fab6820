"""CPU suite: term objectives compiled at run time (lbfgspp_amd.TermObjective, lbfgsx_objective_* of include/lbfgsx.h).
Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object says about its
kernels is read from the code object itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's examples/example-rosenbrock.cpp pair, statement by statement as the built-in ObjRosen
ROSEN = """const T t1 = T(1) - x[0];
const T t2 = T(10) * (x[1] - x[0] * x[0]);
g[1] = T(20) * t2;
g[0] = T(-2) * (x[0] * g[1] + t1);
return t1 * t1 + t2 * t2;"""
# 0.5 (a x - b)^2 with a = p0, b = p1: the built-in ObjQuad (the factor 0.5 inside the term: exact, a power of two)
QUAD = """const T r = p0[i] * x[0] - p1[i];
g[0] = p0[i] * r;
return T(0.5) * (r * r);"""


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body,K", [(ROSEN, 2), (QUAD, 1)], ids=["rosenbrock", "quadratic"])
def test_bodies_compile_to_gfx950_without_scratch_and_are_cached(A, body, K, dtype):
    f = A.TermObjective(body, K=K)
    info = f.info(dtype)
    print(info)
    assert info["scratch_by_kernel"]["k_trial"] == 0 and info["scratch_by_kernel"]["k_eval"] == 0
    assert info["scratch_bytes"] == 0
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    again = A.TermObjective(body, K=K).info(dtype)
    assert again["cache_hit"] and again["compile_ms"] == info["compile_ms"] and again["vgprs"] == info["vgprs"]
    # another dtype or K is another cache entry
    other = A.TermObjective(body + "\n", K=K).info(dtype)
    assert not other["cache_hit"]


def test_code_object_is_for_gfx950(A):
    """the four kernels are in the code object under the names the library looks up, built for gfx950"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    src = A.TermObjective(ROSEN, K=2).source(np.float64)
    for k in ("k_eval<S, ObjTerm>", "k_trial<S, ObjTerm>", "k_b_eval<S, ObjTerm>", "k_b_dg_maxstep_trial<S, ObjTerm>"):
        assert "template __global__ void " + k in src
    assert '#include "lbfgs_kernels.cuh"' in src and '#include "lbfgsb_kernels.cuh"' in src
    assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
    f = A.TermObjective(ROSEN, K=2)  # (the handle lives as long as the object)
    h = f.compile(np.float64)
    assert core.lbfgsx_objective_K(h) == 2 and core.lbfgsx_objective_dtype(h) == L.F64


def test_syntax_error_is_reported_with_its_line_and_nothing_breaks(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    bad = "const T r = x[0];\ng[0] = r\nreturn r * r;"  # line 2 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.TermObjective(bad).compile()
    assert "objective_body:2:" in str(e.value) and "error" in str(e.value)
    h = C.c_void_p()
    log = C.create_string_buffer(4096)
    rc = core.lbfgsx_objective_compile(C.byref(h), L.F64, 1, bad.encode(), log, len(log))
    assert rc == L.E_INVALID and not h.value and b"objective_body:2:" in log.value
    rc = core.lbfgsx_objective_compile(C.byref(h), L.F64, 1, b"T q = undeclared_name;\nreturn q;", log, len(log))
    assert rc == L.E_INVALID and b"objective_body:1:" in log.value and b"undeclared_name" in log.value
    # the process goes on: a correct body compiles afterwards
    good = A.TermObjective("g[0] = x[0];\nreturn T(0.5) * (x[0] * x[0]);")
    assert good.info()["scratch_bytes"] == 0


def test_body_with_inline_assembly_is_refused(A):
    """the contract of a body excludes inline assembly; the word alone is enough to refuse it, before any compilation"""
    word = "as" + "m"
    for body in ("%s volatile(\"\");\ng[0] = x[0];\nreturn x[0];" % word, "g[0] = x[0]; __%s__(\"\"); return x[0];" % word):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.TermObjective(body).compile()


def test_limits_are_named(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    with pytest.raises(ValueError, match="K = 3 is not supported.*K = 1 or K = 2"):
        A.TermObjective(ROSEN, K=3)
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    assert core.lbfgsx_objective_compile(C.byref(h), L.F64, 3, ROSEN.encode(), log, len(log)) == L.E_INVALID
    assert b"K = 3" in log.value and b"K = 1 or K = 2" in log.value
    five = [np.ones(4)] * 5
    with pytest.raises(ValueError, match="5 data arrays given, at most 4"):
        A.TermObjective(QUAD, data=five)
    with pytest.raises(ValueError, match="9 scalars given, at most 8"):
        A.TermObjective(QUAD, scalars=range(9))
    # n not a multiple of K: Python and the C entry point, before anything touches a device
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="n = 5 is not a multiple of K = 2"):
        s.minimize(A.TermObjective(ROSEN, K=2), np.zeros(5))
    f = A.TermObjective(ROSEN, K=2)
    hobj = f.compile()
    res = L.Result()
    x = np.zeros(5)
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hobj, 5, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"n = 5 is not a multiple of K = 2" in res.msg
    # an objective compiled for the other dtype
    h32 = f.compile(np.float32)
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h32, 6, None, 0, None, None, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"other dtype" in res.msg
    with pytest.raises(ValueError, match="must have 6 elements"):
        s.minimize(A.TermObjective(QUAD, data=(np.ones(6), np.ones(5))), np.zeros(6))


NEW_SYMBOLS = {"liblbfgsx.so": ["lbfgsx_objective_compile", "lbfgsx_objective_destroy", "lbfgsx_objective_source",
                                "lbfgsx_objective_info", "lbfgsx_objective_K", "lbfgsx_objective_dtype", "lbfgsx_objective_bind",
                                "lbfgsx_objective_upload", "lbfgsx_objective_bound"],
               "liblbfgsx_solver.so": ["lbfgsx_solver_minimize_obj"]}


def test_new_symbols_are_exported_and_listed(A):
    listed = open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "export.map")).read()
    for lib, names in NEW_SYMBOLS.items():
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lbfgspp_amd", lib)], stdout=subprocess.PIPE,
                             text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for name in names:
            assert name in exported, "%s does not export %s" % (lib, name)
            assert name + ";" in listed, "export.map does not list %s" % name
    header = open(os.path.join(ROOT, "include", "lbfgsx.h")).read() + open(os.path.join(ROOT, "include", "lbfgsx_solver.h")).read()
    for names in NEW_SYMBOLS.values():
        for name in names:
            assert name + "(" in header


def test_minimize_obj_without_a_gpu_answers_nogpu(A):
    """as tests/test_abi_cpu.py::test_no_silent_cpu_fallback for its siblings; with a GPU this test is a no-op"""
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    if core.lbfgsx_device_count() > 0:
        pytest.skip("GPU present")
    f = A.TermObjective(ROSEN, K=2)
    for s, extra in ((A.LBFGSSolver(A.LBFGSParam()), ()), (A.LBFGSBSolver(A.LBFGSBParam()), (-np.ones(10), np.ones(10)))):
        with pytest.raises(RuntimeError, match="no HIP device"):
            s.minimize(f, np.zeros(10), *extra)
        assert s.last.status == L.E_NOGPU
    # binding needs a context, and no context can exist
    h = C.c_void_p()
    assert core.lbfgsx_create(C.byref(h), 0, 16, 3, 0, 0) == L.E_NOGPU
    assert core.lbfgsx_objective_bind(None, f.compile(), None, None, None) == L.E_INVALID


def test_generated_wrapper_names_no_forbidden_instruction(A):
    """the text the library generates around a body holds no scalar store, scalar atomic or scalar-cache instruction name and
    no inline assembly of its own (a plain substring check; the names are spelt in pieces so that this file does not hold
    them either)"""
    s = "s" + "_"
    banned = [s + "store", s + "buffer" + "_store", s + "scratch" + "_store", s + "atomic", s + "buffer" + "_atomic",
              s + "dcache" + "_wb", s + "dcache" + "_discard", "as" + "m(", "as" + "m volatile", "__as" + "m"]
    for body, K in ((ROSEN, 2), (QUAD, 1)):
        for dtype in (np.float64, np.float32):
            text = A.TermObjective(body, K=K).source(dtype)
            assert body in text and len(text) > len(body) + 500
            low = text.lower()
            for word in banned:
                assert word not in low, word
