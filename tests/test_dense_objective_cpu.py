"""CPU suite: dense linear-model objectives compiled at run time (lbfgspp_amd.DenseLinearObjective,
lbfgsx_objective_compile_dense of include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target
gfx950, what the code object says about its kernels is read from the code object itself, and the numpy restatement
(tests/dense_ref.py) is checked against plain dense arithmetic and against the sparse forms' restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dense_ref as DR
import linear_ref as LR
import multilinear_ref as MR
from test_multilinear_objective_cpu import SOFTMAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_dense_eval", "k_dense_trial", "k_dense_b_eval", "k_dense_b_dg_maxstep_trial", "k_dense_rows", "k_dense_rows_trial",
           "k_dense_partials")
EXPORTS = ("lbfgsx_objective_compile_dense", "lbfgsx_objective_source_dense", "lbfgsx_objective_bind_dense",
           "lbfgsx_objective_dense_info", "lbfgsx_objective_dense_read", "lbfgsx_solver_minimize_dense")
ONE = np.ones((1, 1))
DIMS = (1, 2, 3, 5, 10, 16)


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


# ---------------------------------------------------------------- the reference module's self-checks
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_agrees_with_plain_dense_arithmetic_to_rounding(dtype):
    """Z against A @ X and the gradient against A^T W in float64 from the same rounded inputs: a sum of k rounded products in
    some order differs from the exact one by at most gamma(k) sum |terms| <= 2 k u sum |terms| for k u < 1/2 (Higham, Accuracy
    and Stability, section 3.1); the float64 product's own error is u64-sized and is covered by the factor 2.  C and L are
    parameters of the restatement: the bound holds for each"""
    u = float(np.finfo(dtype).eps) / 2
    for name in ("f3", "f65", "pad", "wide16"):
        for Cc in (256, 7):
            P = DR.problem(name, dtype, C=Cc)
            x = np.random.default_rng(4).standard_normal(P.n).astype(dtype)
            A64, X = P.A.astype(np.float64), x.reshape(P.F, P.D).astype(np.float64)
            for L in (1, 4, 64):
                Z = P.z(x, L)
                assert Z.dtype == dtype and Z.shape == (P.R, P.D)
                assert (np.abs(Z - A64 @ X) <= 2 * P.F * u * (np.abs(A64) @ np.abs(X)) + 1e-300).all(), (name, L)
            for ridge in (False, True):
                g, terms, W, v, part = P.evaluate(x, DR.lanes_rule(P.F), "coupled", ridge)
                assert g.dtype == dtype and part.shape == (-(-P.R // Cc), P.F, P.D) and W.shape == (P.R, P.D)
                assert terms.size == P.R + (P.n if ridge else 0)
                W64 = W.astype(np.float64)
                psi = LR.ridge(x, P.c0)[0].astype(np.float64).reshape(P.F, P.D) if ridge else 0
                want = A64.T @ W64 + psi
                bound = 2 * (P.R + 1) * u * (np.abs(A64).T @ np.abs(W64) + np.abs(psi))
                assert (np.abs(g.reshape(P.F, P.D) - want) <= bound + 1e-300).all(), (name, Cc)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_sums_are_the_sparse_restatement_on_the_full_csr_matrix(dtype):
    for name in ("f1", "f3", "f65", "f257", "pad"):
        P = DR.problem(name, dtype)
        x = np.random.default_rng(5).standard_normal(P.n).astype(dtype)
        rp, col, val = P.csr()
        for L in (1, 2, 8, 64):
            assert P.z(x, L).tobytes() == MR.row_sums(rp, col, val, x.reshape(P.F, P.D), L).tobytes(), (name, L)
        assert DR.lanes_rule(P.F) == LR.lanes_rule(P.R, P.R * P.F)
    assert [DR.lanes_rule(F) for F in (1, 2, 3, 63, 64, 65, 1000)] == [1, 2, 2, 32, 64, 64, 64]


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_test_body_compiles_with_zero_scratch_at_every_dimension(A, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for D in DIMS:
        for name, row in (("coupled", MR.COUPLED), ("mhinge", MR.MHINGE), ("softmax", SOFTMAX)):
            for coord in (None, MR.RIDGE):
                f = A.DenseLinearObjective(row, ONE, D, coord_body=coord)
                info = f.info(dtype)
                print("%s D %d %s ridge %s: vgprs %d scratch %d" % (np.dtype(dtype).name, D, name, coord is not None, info["vgprs"],
                                                                    info["scratch_bytes"]))
                # the two maxima cover the row passes and the partial pass as well as the four column-pass kernels
                assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values()), (name, D)
                assert 0 < info["vgprs"] <= 256
                h = f.compile(dtype)
                assert core.lbfgsx_objective_form(h) == 7 and core.lbfgsx_objective_K(h) == 1
                assert core.lbfgsx_objective_dim(h) == D
                assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)
    # D enters the cache key: the same texts at another D are another code object, at the same D the cached one
    assert A.DenseLinearObjective(MR.COUPLED, ONE, 3).info(dtype)["cache_hit"]
    fresh = A.DenseLinearObjective(MR.COUPLED + "\n// seven", ONE, 7).info(dtype)
    again = A.DenseLinearObjective(MR.COUPLED + "\n// seven", ONE, 7).info(dtype)
    other = A.DenseLinearObjective(MR.COUPLED + "\n// seven", ONE, 6).info(dtype)
    assert not fresh["cache_hit"] and again["cache_hit"] and not other["cache_hit"]


def test_generated_source_names_both_bodies_the_dimension_and_the_seven_kernels(A):
    for dtype in (np.float64, np.float32):
        src = A.DenseLinearObjective(MR.MHINGE, ONE, 5, coord_body=MR.RIDGE).source(dtype)
        assert src.count(MR.MHINGE) == 1 and src.count(MR.RIDGE) == 1
        assert "static constexpr int D = 5;" in src and "static constexpr int K = 1;" in src
        assert '#line 1 "row_body"' in src and '#line 1 "coord_body"' in src and "kCoord = true" in src
        assert '#include "linear_dense_kernels.cuh"' in src and "struct ObjDense" in src
        assert "const T* A;" in src and "int64_t R, F, lda, chunks;" in src and "colptr" not in src
        assert "row(const T (&z)[D], T (&dz)[D], int64_t r)" in src and "coord(const T (&x)[1], T (&g)[1], int64_t i)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjDense>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    src = A.DenseLinearObjective(MR.MHINGE, ONE, 16).source()
    assert "static constexpr int D = 16;" in src and "kCoord = false" in src and MR.RIDGE not in src
    # the other forms' units name none of the new kernels
    assert "k_dense" not in A.MultiLinearObjective(MR.MHINGE, (np.array([0, 1]), np.array([0]), np.array([1.0])), 1, 5).source()


def test_exports_the_form_number_and_the_class_are_declared(A):
    with open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "export.map")) as f:
        listed = set(re.findall(r"\blbfgsx_\w+", f.read()))
    with open(os.path.join(ROOT, "include", "lbfgsx.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "lbfgsx_solver.h")) as f:
        header += f.read()
    core, sol = A.load()
    for name in EXPORTS:
        assert name in listed and re.search(r"\b%s\(" % name, header), name
        assert hasattr(sol if "solver" in name else core, name)
    assert re.search(r"\bLBFGSX_FORM_DENSE = 7\b", header)
    assert "DenseLinearObjective" in A.__all__ and issubclass(A.DenseLinearObjective, A.TermObjective)
    for text in (header,):
        for m in re.finditer(r"Not built:[^/]*?\*/", text, re.S):
            assert "dense A" not in m.group(0)


# ---------------------------------------------------------------- refusals made before any device work
def test_refusals_before_any_device_work_name_the_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for D in (0, 17, -3):
        h = C.c_void_p()
        log = C.create_string_buffer(4096)
        rc = core.lbfgsx_objective_compile_dense(C.byref(h), L.F64, D, None, MR.COUPLED.encode(), log, len(log))
        what = "dense linear-model objective: D = %d is not supported: a row has D = 1 .. 16 outputs" % D
        assert rc == L.E_INVALID and not h.value and log.value.decode() == what
        assert core.lbfgsx_objective_source_dense(L.F64, D, None, MR.COUPLED.encode(), None, 0) == L.E_INVALID
        assert L.last_error() == what
        with pytest.raises(ValueError, match="D = %d is not supported: a row has D = 1 .. 16 outputs" % D):
            A.DenseLinearObjective(MR.COUPLED, ONE, D)
    for row, coord, noun in (("asm volatile(\"\"); return z[0];", None, "row body"), (MR.COUPLED, "asm(\"\"); return x[0];", "coordinate body")):
        h = C.c_void_p()
        log = C.create_string_buffer(4096)
        rc = core.lbfgsx_objective_compile_dense(C.byref(h), L.F64, 3, coord.encode() if coord else None, row.encode(), log, len(log))
        assert rc == L.E_INVALID and not h.value
        assert "dense linear-model objective: the %s contains 'asm'" % noun in log.value.decode()
        with pytest.raises(ValueError, match="the %s contains 'asm'" % noun):
            A.DenseLinearObjective(row, ONE, 3, coord_body=coord).compile()
    for body in (b"", None):
        h = C.c_void_p()
        log = C.create_string_buffer(4096)
        assert core.lbfgsx_objective_compile_dense(C.byref(h), L.F64, 3, None, body, log, len(log)) == L.E_INVALID
        assert "dense linear-model objective: empty row body" in log.value.decode() and not h.value
    # the Python class: x has to hold whole weight rows, F of them
    f = A.DenseLinearObjective(MR.COUPLED, np.ones((4, 2)), 3)
    with pytest.raises(ValueError, match="n = 4 is not a multiple of D = 3"):
        f._check_n(4)
    with pytest.raises(ValueError, match="n = 2 \\* 3 = 6 weights and x has 9 elements"):
        f._check_n(9)
    f._check_n(6)
    assert (f.R, f.F, f.n, f.lda) == (4, 2, 6, 2) and f._data_sizes(6) == (6, 2, 4, 12) and not f.on_device
    with pytest.raises(ValueError, match="n = 7 is not a multiple of D = 3"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(7))
    with pytest.raises(ValueError, match="2-D array of numbers"):
        A.DenseLinearObjective(MR.COUPLED, np.ones(4), 3)
    with pytest.raises(ValueError, match="shape \\(0, 2\\)"):
        A.DenseLinearObjective(MR.COUPLED, np.ones((0, 2)), 3)
    with pytest.raises(ValueError, match="lanes = 3"):
        A.DenseLinearObjective(MR.COUPLED, ONE, 3, lanes=3)
    # a compile error is reported against the body's own lines
    with pytest.raises(ValueError, match="row_body"):
        A.DenseLinearObjective("return z[0] + nothing_of_that_name;", ONE, 2).compile()
    # the C entry points of the solvers say what is wrong with the request before any device work
    s = A.LBFGSSolver(A.LBFGSParam())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    mat, x = np.ones((2, 3)), np.zeros(7)

    def call(handle, n, R, Aptr, lda):
        res = L.Result()
        rc = sol.lbfgsx_solver_minimize_dense(s._h, handle, n, R, Aptr, lda, 0, 0, None, 0, None, None, vp(x), None, None, None,
                                              C.byref(res))
        return rc, res.msg.decode()
    h = f.compile()
    for args, what in (((h, 7, 2, vp(mat), 3), "dense linear-model objective: n = 7 is not a multiple of D = 3"),
                       ((h, 6, 0, vp(mat), 3), "dense linear-model objective: R = 0"),
                       ((h, 6, 2, None, 3), "dense linear-model objective: A is null"),
                       ((h, 6, 2, vp(mat), 1), "dense linear-model objective: lda = 1 is less than F = n / D = 2")):
        rc, msg = call(*args)
        assert rc == L.E_INVALID and what in msg, msg
    multi = A.MultiLinearObjective(MR.COUPLED, (np.array([0, 1]), np.array([0]), np.array([1.0])), 1, 3)  # owns its handle
    rc, msg = call(multi.compile(), 6, 2, vp(mat), 3)
    assert rc == L.E_INVALID and "the handle is not a dense linear-model objective (lbfgsx_objective_compile_dense)" in msg
    # and the other two minimise calls refuse a dense handle
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h, 6, None, 0, None, vp(x), None, None, None, C.byref(res))
    assert rc == L.E_INVALID and "a dense linear-model objective is minimised with its matrix: lbfgsx_solver_minimize_dense" in res.msg.decode()
    rp, col, val = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0])
    rc = sol.lbfgsx_solver_minimize_linear(s._h, h, 6, 1, 1, vp(rp), vp(col), vp(val), 0, 0, None, 0, None, None, vp(x), None, None,
                                           None, C.byref(res))
    assert rc == L.E_INVALID and "the handle is not a linear-model objective" in res.msg.decode()
