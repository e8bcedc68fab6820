"""CPU suite: multi-output linear-model objectives compiled at run time (lbfgspp_amd.MultiLinearObjective,
lbfgsx_objective_compile_linear_multi of include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the
fixed target gfx950, what the code object says about its kernels is read from the code object itself, and the numpy
restatement (tests/multilinear_ref.py) is checked against dense arithmetic and against the scalar form's restatement."""
import ctypes as C

import numpy as np
import pytest

import linear_ref as LR
import multilinear_ref as MR

KERNELS = ("k_linm_eval", "k_linm_trial", "k_linm_b_eval", "k_linm_b_dg_maxstep_trial", "k_linm_rows", "k_linm_rows_trial")
ONE = (np.array([0, 1]), np.array([0]), np.array([1.0]))  # the 1 x 1 matrix
DIMS = (1, 2, 3, 5, 10, 16)
# softmax cross-entropy with the label y = int(p0[r]), loops written with #pragma unroll
SOFTMAX = """
T m = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    m = z[k] > m ? z[k] : m;
T e[D];
T s = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    e[k] = exp(z[k] - m);
    s = s + e[k];
}
const int y = int(p0[r]);
T zy = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    zy = k == y ? z[k] : zy;
#pragma unroll
for (int k = 0; k < D; k++)
    dz[k] = c[1] * (e[k] / s - (k == y ? T(1) : T(0)));
return c[1] * ((log(s) + m) - zy);"""


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


# ---------------------------------------------------------------- the reference module's self-checks
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_agrees_with_dense_arithmetic_to_rounding(dtype):
    """Z against A @ X and the gradient against A^T W in float64 from the same rounded inputs: a sum of k rounded products in
    some order differs from the exact one by at most gamma(k) sum |terms| <= 2 k u sum |terms| for k u < 1/2 (Higham, Accuracy
    and Stability, section 3.1); the float64 dense product's own error is u64-sized and is covered by the factor 2"""
    u = float(np.finfo(dtype).eps) / 2
    for name in ("tiny", "random", "wide16"):
        M = MR.problem(name, dtype)
        x = np.random.default_rng(4).standard_normal(M.n).astype(dtype)
        dense = np.zeros((M.R, M.F))
        rows = np.repeat(np.arange(M.R), np.diff(M.rowptr))
        np.add.at(dense, (rows, M.col), M.val.astype(np.float64))
        mag = np.zeros((M.R, M.F))
        np.add.at(mag, (rows, M.col), np.abs(M.val.astype(np.float64)))
        X = x.reshape(M.F, M.D).astype(np.float64)
        klen = int(np.diff(M.rowptr).max())
        for L in (1, 4, 64):
            Z = M.z(x, L)
            assert Z.dtype == dtype and Z.shape == (M.R, M.D)
            assert (np.abs(Z - dense @ X) <= 2 * klen * u * (mag @ np.abs(X)) + 1e-300).all(), (name, L)
        W, _ = MR.coupled(M.z(x, 4), M.targets, M.c1)
        pg, _ = LR.ridge(x, M.c0)
        clen = int(np.diff(M.topo[0].astype(np.int64)).max()) + 1
        for psi in (None, pg.reshape(M.F, M.D)):
            g = MR.gradient(W, M.val, M.topo, M.F, M.C, psi)
            want = dense.T @ W.astype(np.float64) + (0 if psi is None else psi.astype(np.float64))
            bound = 2 * clen * u * (mag.T @ np.abs(W.astype(np.float64)) + (0 if psi is None else np.abs(psi)))
            assert g.dtype == dtype and (np.abs(g - want) <= bound + 1e-300).all(), name
            empty = np.diff(M.topo[0].astype(np.int64)) == 0
            if psi is None and empty.any():
                assert (g[empty] == 0).all() and not np.signbit(g[empty]).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_output_is_the_scalar_restatement_bit_for_bit(dtype):
    for P in (LR.tiny(dtype), LR.random_rows(60, 23, 40, 9, dtype), LR.long_columns(dtype, R=700, n=9, C=256)):
        x = np.random.default_rng(5).standard_normal(P.n).astype(dtype)
        for L in (1, 2, 8, 64):
            z = MR.row_sums(P.rowptr, P.col, P.val, x.reshape(-1, 1), L)
            assert z.shape == (P.R, 1) and z[:, 0].tobytes() == LR.row_sums(P.rowptr, P.col, P.val, x, L).tobytes()
        w, _ = LR.cubic(P.z(x, 8), P.p0)
        pg, _ = LR.ridge(x, P.c0)
        for psi in (None, pg):
            g1 = MR.gradient(w.reshape(-1, 1), P.val, P.topo, P.n, P.C, None if psi is None else psi.reshape(-1, 1))
            assert g1[:, 0].tobytes() == LR.gradient(w, P.val, P.topo, P.n, P.C, psi).tobytes()
    # and each output of a D-output problem is the scalar restatement of its own column of X
    M = MR.problem("random", dtype)
    x = np.random.default_rng(6).standard_normal(M.n).astype(dtype)
    Z = M.z(x, 4)
    for k in range(M.D):
        xk = np.ascontiguousarray(x.reshape(M.F, M.D)[:, k])
        assert Z[:, k].tobytes() == LR.row_sums(M.rowptr, M.col, M.val, xk, 4).tobytes()


def test_the_bodies_twins_are_the_derivatives_of_their_values():
    """central differences in float64 on the numpy twins: dz is the gradient of phi"""
    rng = np.random.default_rng(7)
    R_, D = 40, 5
    Z = rng.standard_normal((R_, D))
    for fn, p0 in ((MR.coupled, rng.standard_normal(R_ * D)), (MR.mhinge, rng.integers(0, D, R_).astype(np.float64))):
        W, _ = fn(Z, p0, 0.125)
        for k in range(D):
            E = np.zeros_like(Z)
            E[:, k] = 1e-6
            num = (fn(Z + E, p0, 0.125)[1] - fn(Z - E, p0, 0.125)[1]) / 2e-6
            assert np.abs(num - W[:, k]).max() <= 1e-7 * max(1.0, np.abs(W).max())
    W, v = MR.mhinge(Z, np.full(R_, 2.0))
    assert (W[:, 2] <= 0).all() and (np.delete(W, 2, axis=1) >= 0).all() and (v >= 0).all()


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_test_body_compiles_with_zero_scratch_at_every_dimension(A, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for D in DIMS:
        for name, row in (("coupled", MR.COUPLED), ("mhinge", MR.MHINGE), ("softmax", SOFTMAX)):
            for coord in (None, MR.RIDGE):
                f = A.MultiLinearObjective(row, ONE, 1, D, coord_body=coord)
                info = f.info(dtype)
                print("%s D %d %s ridge %s: vgprs %d scratch %d" % (np.dtype(dtype).name, D, name, coord is not None, info["vgprs"],
                                                                    info["scratch_bytes"]))
                # the two maxima cover the row passes as well as the four column-pass kernels
                assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values()), (name, D)
                assert 0 < info["vgprs"] <= 256
                h = f.compile(dtype)
                assert core.lbfgsx_objective_form(h) == 6 and core.lbfgsx_objective_K(h) == 1
                assert core.lbfgsx_objective_dim(h) == D
                assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)
    # D enters the cache key: the same texts at another D are another code object, at the same D the cached one
    a = A.MultiLinearObjective(MR.COUPLED, ONE, 1, 3).info(dtype)
    b = A.MultiLinearObjective(MR.COUPLED, ONE, 1, 5).info(dtype)
    assert a["cache_hit"] and b["cache_hit"]
    fresh = A.MultiLinearObjective(MR.COUPLED + "\n// seven", ONE, 1, 7).info(dtype)
    again = A.MultiLinearObjective(MR.COUPLED + "\n// seven", ONE, 1, 7).info(dtype)
    other = A.MultiLinearObjective(MR.COUPLED + "\n// seven", ONE, 1, 6).info(dtype)
    assert not fresh["cache_hit"] and again["cache_hit"] and not other["cache_hit"]


def test_generated_source_names_both_bodies_the_dimension_and_the_six_kernels(A):
    for dtype in (np.float64, np.float32):
        src = A.MultiLinearObjective(MR.MHINGE, ONE, 1, 5, coord_body=MR.RIDGE).source(dtype)
        assert src.count(MR.MHINGE) == 1 and src.count(MR.RIDGE) == 1
        assert "static constexpr int D = 5;" in src and "static constexpr int K = 1;" in src
        assert '#line 1 "row_body"' in src and '#line 1 "coord_body"' in src and "kCoord = true" in src
        assert '#include "linear_multi_kernels.cuh"' in src and "const uint32_t* colptr;" in src
        assert "row(const T (&z)[D], T (&dz)[D], int64_t r)" in src and "coord(const T (&x)[1], T (&g)[1], int64_t i)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjLinearMulti>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    src = A.MultiLinearObjective(MR.MHINGE, ONE, 1, 16).source()
    assert "static constexpr int D = 16;" in src and "kCoord = false" in src and MR.RIDGE not in src


# ---------------------------------------------------------------- refusals made before any device work
def test_refusals_before_any_device_work_name_the_value(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for D in (0, 17, -3):
        h = C.c_void_p()
        log = C.create_string_buffer(4096)
        rc = core.lbfgsx_objective_compile_linear_multi(C.byref(h), L.F64, D, None, MR.COUPLED.encode(), log, len(log))
        what = "multi-output linear-model objective: D = %d is not supported: a row has D = 1 .. 16 outputs" % D
        assert rc == L.E_INVALID and not h.value and log.value.decode() == what
        assert core.lbfgsx_objective_source_linear_multi(L.F64, D, None, MR.COUPLED.encode(), None, 0) == L.E_INVALID
        assert L.last_error() == what
        with pytest.raises(ValueError, match="D = %d is not supported: a row has D = 1 .. 16 outputs" % D):
            A.MultiLinearObjective(MR.COUPLED, ONE, 1, D)
    for row, coord, noun in (("asm volatile(\"\"); return z[0];", None, "row body"), (MR.COUPLED, "asm(\"\"); return x[0];", "coordinate body")):
        h = C.c_void_p()
        log = C.create_string_buffer(4096)
        rc = core.lbfgsx_objective_compile_linear_multi(C.byref(h), L.F64, 3, coord.encode() if coord else None, row.encode(), log,
                                                        len(log))
        assert rc == L.E_INVALID and not h.value
        assert "multi-output linear-model objective: the %s contains 'asm'" % noun in log.value.decode()
        with pytest.raises(ValueError, match="the %s contains 'asm'" % noun):
            A.MultiLinearObjective(row, ONE, 1, 3, coord_body=coord).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(4096)
    assert core.lbfgsx_objective_compile_linear_multi(C.byref(h), L.F64, 3, None, b"", log, len(log)) == L.E_INVALID
    assert "empty row body" in log.value.decode()
    # the Python class: x has to hold whole weight rows, F of them
    f = A.MultiLinearObjective(MR.COUPLED, ONE, 1, 3)
    with pytest.raises(ValueError, match="n = 4 is not a multiple of D = 3"):
        f._check_n(4)
    with pytest.raises(ValueError, match="n = 1 \\* 3 = 3 weights and x has 6 elements"):
        f._check_n(6)
    f._check_n(3)
    assert f.n == 3 and f._data_sizes(3) == (3, 1, 1, 3)
    with pytest.raises(ValueError, match="n = 7 is not a multiple of D = 3"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(7))
    with pytest.raises(ValueError, match="features = 0"):
        A.MultiLinearObjective(MR.COUPLED, ONE, 0, 3)
    # a compile error is reported against the body's own lines
    with pytest.raises(ValueError, match="row_body"):
        A.MultiLinearObjective("return z[0] + nothing_of_that_name;", ONE, 1, 2).compile()
    # the C entry point of the solvers names both values before any device work
    _, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    res = L.Result()
    rp, col, val = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0]))
    x = np.zeros(7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = sol.lbfgsx_solver_minimize_linear(s._h, f.compile(), 7, 1, 1, vp(rp), vp(col), vp(val), 0, 0, None, 0, None, None, vp(x),
                                           None, None, None, C.byref(res))
    assert rc == L.E_INVALID and "n = 7 is not a multiple of D = 3" in res.msg.decode()
