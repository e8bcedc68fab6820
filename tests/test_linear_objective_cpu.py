"""CPU suite: linear-model objectives compiled at run time (lbfgspp_amd.LinearObjective, lbfgsx_objective_compile_linear of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, what the code object
says about its kernels is read from the code object itself, and the numpy restatement (tests/linear_ref.py) is checked
against exact rational arithmetic."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import linear_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_lin_eval", "k_lin_trial", "k_lin_b_eval", "k_lin_b_dg_maxstep_trial", "k_lin_rows", "k_lin_rows_trial")
ONE = (np.array([0, 1]), np.array([0]), np.array([1.0]))  # the 1 x 1 matrix


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


# ---------------------------------------------------------------- the reference module's self-checks
def test_transposed_list_is_stable_and_the_chunk_table_covers_the_long_columns():
    for P in (LR.tiny(np.float64), LR.random_rows(70, 33, 9, 5, np.float64), LR.long_columns(np.float64, R=600, n=11, C=256)):
        colptr, trow, tpos = P.topo
        assert colptr.dtype == np.uint32 and trow.dtype == np.int32 and tpos.dtype == np.uint32
        assert colptr[0] == 0 and colptr[P.n] == P.nnz and sorted(tpos.tolist()) == list(range(P.nnz))
        for j in range(P.n):
            mine = tpos[colptr[j]:colptr[j + 1]].astype(np.int64)
            assert (P.col[mine] == j).all() and (np.diff(mine) > 0).all()  # ascending CSR position: ascending r, caller's order
            assert all(P.rowptr[r] <= k < P.rowptr[r + 1] for r, k in zip(trow[colptr[j]:colptr[j + 1]], mine))
        long_col, long_chunk, chunk = LR.chunk_table(colptr, P.C)
        lens = np.diff(colptr.astype(np.int64))
        assert long_col.tolist() == np.flatnonzero(lens > P.C).tolist() and long_chunk.size == long_col.size + 1
        for s, j in enumerate(long_col):
            mine = chunk[long_chunk[s]:long_chunk[s + 1]]
            assert mine[0, 0] == colptr[j] and mine[-1, 1] == colptr[j + 1] and (mine[1:, 0] == mine[:-1, 1]).all()
            assert (mine[:-1, 1] - mine[:-1, 0] == P.C).all() and 0 < mine[-1, 1] - mine[-1, 0] <= P.C
    tiny = LR.tiny(np.float64)
    assert np.diff(tiny.rowptr).tolist() == [3, 0, 3] and np.diff(tiny.topo[0].astype(np.int64)).tolist() == [2, 1, 0, 2, 1]
    assert tiny.topo[2][tiny.topo[0][3]:tiny.topo[0][4]].tolist() == [0, 2]  # the duplicate (0, 3), in the caller's order
    big = LR.long_columns(np.float64)
    lens = np.diff(big.topo[0].astype(np.int64))
    assert (big.R, big.n, lens[0], lens[5], lens[36]) == (9000, 37, 9000, 4096, 4097) and big.has_long()
    assert LR.chunk_table(big.topo[0])[0].tolist() == [0, 36] and LR.chunk_table(big.topo[0])[1].tolist() == [0, 3, 5]


def test_the_lanes_rule():
    assert [LR.lanes_rule(10, k) for k in (1, 10, 19, 20, 39, 40, 79, 80, 640, 1280, 10 ** 6)] == [1, 1, 1, 2, 2, 4, 4, 8, 64, 64, 64]


def _gamma(k, dt):
    u = float(np.finfo(dt).eps) / 2
    return Fraction(k * u) / (1 - Fraction(k * u))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_agrees_with_exact_sums_within_the_bound_of_its_lengths(dtype):
    """z_r is a sum of len_r rounded products through at most len_r - 1 rounded additions in SOME order, so
    |z_r - exact| <= gamma(len_r) * sum |val x|, gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability, section 3.1), for
    every L.  grad[j], with the restatement's own w taken as exact input, is psi' plus len_j rounded products through at most
    len_j rounded additions (lanes, halving and chunk partials are all just another order):
    |grad[j] - exact| <= gamma(len_j + 1) * (|psi'| + sum |val w|)."""
    for P in (LR.tiny(dtype), LR.random_rows(60, 23, 40, 9, dtype), LR.long_columns(dtype, R=700, n=9, C=256)):
        rng = np.random.default_rng(4)
        x = rng.standard_normal(P.n).astype(dtype)
        fr = lambda a: [Fraction(float(v)) for v in a]
        fx, fval = fr(x), fr(P.val)
        for L in (1, 2, 8, 64):
            z = P.z(x, L)
            for r in range(P.R):
                ks = range(P.rowptr[r], P.rowptr[r + 1])
                exact = sum((fval[k] * fx[P.col[k]] for k in ks), Fraction(0))
                mag = sum((abs(fval[k] * fx[P.col[k]]) for k in ks), Fraction(0))
                assert abs(Fraction(float(z[r])) - exact) <= _gamma(len(ks), dtype) * mag, (L, r)
        w, _ = LR.cubic(P.z(x, 8), P.p0)
        pg, _ = LR.ridge(x, P.c0)
        fw = fr(w)
        colptr, trow, tpos = P.topo
        for psi in (None, pg):
            g = LR.gradient(w, P.val, P.topo, P.n, P.C, psi)
            for j in range(P.n):
                qs = range(colptr[j], colptr[j + 1])
                terms = [fval[tpos[q]] * fw[trow[q]] for q in qs] + ([Fraction(float(psi[j]))] if psi is not None else [])
                bound = _gamma(len(qs) + 1, dtype) * sum((abs(t) for t in terms), Fraction(0))
                assert abs(Fraction(float(g[j])) - sum(terms, Fraction(0))) <= bound, j
                if not terms:
                    assert g[j] == 0 and not np.signbit(g[j])


def test_an_empty_lane_holds_plus_zero_and_sums_start_from_the_first_contribution():
    dt = np.float64
    # one row, one entry whose product is -0: with L = 2 lane 1 holds +0 and z = -0 + +0 = +0; with L = 1 z = -0
    z1 = LR.row_sums(np.array([0, 1]), np.array([0]), np.array([-1.0]), np.array([0.0]), 1)
    z2 = LR.row_sums(np.array([0, 1]), np.array([0]), np.array([-1.0]), np.array([0.0]), 2)
    assert np.signbit(z1[0]) and not np.signbit(z2[0])
    topo = LR.transpose(np.array([0, 1]), np.array([0]), 2)
    g = LR.gradient(np.array([0.0]), np.array([-1.0]), topo, 2)
    assert np.signbit(g[0]) and g[1] == 0 and not np.signbit(g[1])  # no leading 0 +; a column with no entry gets +0
    part = LR.chunk_partial(np.array([-0.0], dt))  # thread 0 holds -0, thread 128 holds +0: the halving gives +0
    assert part == 0 and not np.signbit(part)


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_both_dtypes_compile_with_zero_scratch_in_all_six_kernels(A, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for name, row in (("cubic", LR.CUBIC), ("hinge", LR.HINGE), ("square", LR.SQUARE), ("logistic", LR.LOGISTIC)):
        for coord in (None, LR.RIDGE):
            f = A.LinearObjective(row, ONE, 1, coord_body=coord)
            info = f.info(dtype)
            print("%s %s ridge %s: vgprs %d scratch %d" % (np.dtype(dtype).name, name, coord is not None, info["vgprs"],
                                                           info["scratch_bytes"]))
            # the two maxima cover the row passes as well as the four column-pass kernels
            assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values()), name
            assert 0 < info["vgprs"] <= 128 and info["compile_ms"] > 0
            h = f.compile(dtype)
            assert core.lbfgsx_objective_form(h) == 5 and core.lbfgsx_objective_K(h) == 1
            assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_names_both_bodies_and_the_six_kernels(A):
    for dtype in (np.float64, np.float32):
        src = A.LinearObjective(LR.HINGE, ONE, 1, coord_body=LR.RIDGE).source(dtype)
        assert src.count(LR.HINGE) == 1 and src.count(LR.RIDGE) == 1
        assert '#line 1 "row_body"' in src and '#line 1 "coord_body"' in src and "kCoord = true" in src
        assert '#include "linear_kernels.cuh"' in src and "const uint32_t* colptr;" in src and "const int32_t* rowptr;" in src
        assert "row(const T z, T& dz, int64_t r)" in src and "coord(const T (&x)[1], T (&g)[1], int64_t i)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjLinear>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    for coord in (None, ""):
        src = A.LinearObjective(LR.HINGE, ONE, 1, coord_body=coord).source()
        assert "kCoord = false" in src and '"coord_body"' not in src and src.count(LR.HINGE) == 1


def test_the_cache_is_keyed_by_form_both_bodies_and_dtype(A):
    row = "dz = z;\nreturn T(0.5) * (z * z);\n// cache test of the linear form"
    coord = "g[0] = x[0]; return T(0.5) * (x[0] * x[0]);\n// cache test of the linear form"
    first = A.LinearObjective(row, ONE, 1).info()
    assert not first["cache_hit"]
    P = LR.tiny(np.float64)
    again = A.LinearObjective(row, (P.rowptr, P.col, P.val), P.n, lanes=8).info()  # the matrix and lanes are not part of the key
    assert again["cache_hit"] and again["compile_ms"] == first["compile_ms"] and again["vgprs"] == first["vgprs"]
    assert not A.LinearObjective(row, ONE, 1, coord_body=coord).info()["cache_hit"]  # the coordinate body is
    assert A.LinearObjective(row, ONE, 1, coord_body=coord).info()["cache_hit"]
    assert not A.LinearObjective(row, ONE, 1).info(np.float32)["cache_hit"]


def test_compile_errors_name_the_body_and_its_line(A):
    bad_row = "const T u = z - p0[r];\ndz = u\nreturn u * u;"     # line 2 lacks its semicolon
    bad_coord = "const T q = x[0]\ng[0] = q;\nreturn q * q;"       # line 1 does
    with pytest.raises(ValueError) as e:
        A.LinearObjective(bad_row, ONE, 1, coord_body=LR.RIDGE).compile()
    assert "LinearObjective" in str(e.value) and "row_body:2:" in str(e.value) and "coord_body:" not in str(e.value)
    with pytest.raises(ValueError) as e:
        A.LinearObjective(LR.HINGE, ONE, 1, coord_body=bad_coord).compile()
    assert "coord_body:1:" in str(e.value) and "row_body:" not in str(e.value) and "error" in str(e.value)


def test_refused_requests_name_the_value(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    with pytest.raises(ValueError, match="the row body contains .* inline assembly is not accepted"):
        A.LinearObjective("%s volatile(\"\");\ndz = z;\nreturn z;" % word, ONE, 1).compile()
    with pytest.raises(ValueError, match="the coordinate body contains .* inline assembly is not accepted"):
        A.LinearObjective(LR.HINGE, ONE, 1, coord_body="g[0] = x[0]; __%s__(\"\"); return x[0];" % word).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    assert core.lbfgsx_objective_compile_linear(C.byref(h), L.F64, None, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"linear-model objective: empty row body" in log.value
    assert core.lbfgsx_objective_source_linear(L.F64, None, b"", None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_linear(C.byref(h), 7, None, LR.HINGE.encode(), log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


# ---------------------------------------------------------------- the Python class
def test_python_side_value_errors(A):
    rp, col, val = np.array([0, 2, 3]), np.array([0, 1, 1]), np.ones(3)
    with pytest.raises(ValueError, match="matrix must be a triple"):
        A.LinearObjective(LR.HINGE, (rp, col), 2)
    with pytest.raises(ValueError, match="rowptr must be a 1-D integer array, not float64"):
        A.LinearObjective(LR.HINGE, (rp.astype(float), col, val), 2)
    with pytest.raises(ValueError, match="col holds 4294967296, which does not fit 32 bits"):
        A.LinearObjective(LR.HINGE, (rp, np.array([0, 1, 2 ** 32]), val), 2)
    with pytest.raises(ValueError, match="col has 3 elements and val has 2"):
        A.LinearObjective(LR.HINGE, (rp, col, np.ones(2)), 2)
    with pytest.raises(ValueError, match="rowptr\\[0\\] = 0 and rowptr\\[R\\] = 2: rowptr starts at 0 and ends at nnz = 3"):
        A.LinearObjective(LR.HINGE, (np.array([0, 1, 2]), col, val), 2)
    with pytest.raises(ValueError, match="rowptr has 1 elements"):
        A.LinearObjective(LR.HINGE, (np.array([0]), col, val), 2)
    with pytest.raises(ValueError, match="nnz = 0"):
        A.LinearObjective(LR.HINGE, (np.array([0, 0]), np.zeros(0, int), np.zeros(0)), 2)
    with pytest.raises(ValueError, match="lanes = 3"):
        A.LinearObjective(LR.HINGE, (rp, col, val), 2, lanes=3)
    with pytest.raises(ValueError, match="lanes = 128"):
        A.LinearObjective(LR.HINGE, (rp, col, val), 2, lanes=128)
    with pytest.raises(ValueError, match="n = 0"):
        A.LinearObjective(LR.HINGE, (rp, col, val), 0)
    with pytest.raises(ValueError, match="LinearObjective: 5 data arrays given, at most 4"):
        A.LinearObjective(LR.HINGE, (rp, col, val), 2, data=[np.ones(2)] * 5)
    f = A.LinearObjective(LR.HINGE, (rp.astype(np.uint8), col.astype(np.int64), [1, 2, 3]), 2, data=(np.ones(2),))
    assert f.rowptr.dtype == np.int32 and f.col.dtype == np.int32 and (f.R, f.nnz, f.n, f.lanes) == (2, 3, 2, 0)
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="the matrix has n = 2 columns and x has 7 elements"):
        s.minimize(f, np.zeros(7))
    f3 = A.LinearObjective(LR.HINGE, (np.array([0, 1, 2, 3]), col, val), 2, data=(np.ones(5),))  # n = 2, R = 3: neither
    with pytest.raises(ValueError, match="LinearObjective: data\\[0\\] must have 2 or 3 elements"):
        s.minimize(f3, np.zeros(2))


def test_the_solver_entry_points_refuse_by_form_before_a_device_is_needed(A):
    from lbfgspp_amd import _lib as L
    _, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    fl = A.LinearObjective(LR.HINGE, ONE, 1)  # the handles live as long as their objects
    fg = A.GraphObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", edges=(np.array([0]), np.array([1])))
    hl, hg = fl.compile(), fg.compile()
    x = np.zeros(2)
    xp = x.ctypes.data_as(C.c_void_p)
    rp, cp, vp = (a.ctypes.data_as(C.c_void_p) for a in (np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1)))
    i32p = C.POINTER(C.c_int32)
    e0 = np.zeros(1, np.int32).ctypes.data_as(i32p)
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hl, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"lbfgsx_solver_minimize_linear" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, hl, 2, 1, e0, e0, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a graph objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, hl, 2, 1, e0, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a mesh objective" in res.msg

    def linear(h, n=2, R=1, nnz=1):
        return sol.lbfgsx_solver_minimize_linear(s._h, h, n, R, nnz, rp, cp, vp, 0, 0, None, 0, None, None, xp, None, None, None,
                                                 C.byref(res))
    assert linear(hg) == L.E_INVALID and b"not a linear-model objective" in res.msg
    assert linear(hl, R=0) == L.E_INVALID and b"R = 0, nnz = 1" in res.msg
    assert linear(hl, nnz=0) == L.E_INVALID and b"R = 1, nnz = 0" in res.msg
    assert linear(fl.compile(np.float32)) == L.E_INVALID and b"the other dtype" in res.msg


NEW_CORE = ["lbfgsx_objective_compile_linear", "lbfgsx_objective_source_linear", "lbfgsx_objective_bind_linear",
            "lbfgsx_objective_linear_topology"]
NEW_SOLVER = ["lbfgsx_solver_minimize_linear"]


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
    assert re.search(r"LBFGSX_FORM_MESH = 4\b", text) and re.search(r"LBFGSX_FORM_LINEAR = 5\b", text)
    assert "LinearObjective" in A.__all__


def test_the_cpp_class_compiles_against_include(tmp_path):
    """LinearObjective<Scalar> of include/LBFGSpp/Device.h in both solvers' minimize, built with g++ against include/"""
    src = tmp_path / "linear_use.cpp"
    src.write_text("""#include <vector>
#include <LBFGS.h>
#include <LBFGSB.h>
using namespace LBFGSpp;
template <class S> S run(const char* row, const char* coord)
{
    std::vector<std::int32_t> rp = {0, 1}, col = {0};
    std::vector<S> val = {S(1)}, y = {S(1)};
    LinearObjective<S> f(row, coord);
    f.matrix(1, 1, rp.data(), col.data(), val.data()).host_data(0, y.data(), 1).scalars({0.5});
    Eigen::Matrix<S, Eigen::Dynamic, 1> x = Eigen::Matrix<S, Eigen::Dynamic, 1>::Zero(1), lb = x, ub = x;
    S fx = 0, fb = 0;
    LBFGSParam<S> p;
    LBFGSSolver<S> s(p);
    s.minimize(f, x, fx);
    LBFGSBParam<S> pb;
    LBFGSBSolver<S> sb(pb);
    sb.minimize(f, x, fb, lb, ub);
    return fx + fb;
}
int main(int argc, char** argv) { return argc > 5 ? int(run<double>(argv[1], argv[2]) + run<float>(argv[1], argv[2])) : 0; }
""")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "oracle", "eigen_shim"), str(src), "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o",
           str(tmp_path / "linear_use")]
    subprocess.run(cmd, check=True)


def test_the_probe_compiles_against_include_as_a_device_build(tmp_path):
    """tests/cpp/linear_probe.cpp with LinearObjective<double> in place of the functor, built with g++ against include/; the
    fixture it is compared with holds data only"""
    import json
    exe = str(tmp_path / "linear_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DLINEAR_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "linear_probe.cpp"),
           "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o", exe]
    subprocess.run(cmd, check=True)
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "linear_probe.cpp")).read()
    for body in (LR.HINGE, LR.RIDGE, LR.SQUARE):  # the probe holds the bodies line by line
        for line in body.strip().splitlines():
            assert '"%s' % line in src, line
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "linear_golden.json")))
    assert set(g) == {"tolerance", "constants", "instances"} and g["tolerance"] == 1e-10
    assert sorted((i["solver"], i["R"], i["n"]) for i in g["instances"]) == [("lbfgs", 120, 40), ("lbfgs", 600, 150),
                                                                             ("lbfgsb", 120, 40), ("lbfgsb", 600, 150)]
    for i in g["instances"]:
        assert i["iterations"] >= 8 and len(i["x_f8_base64"]) == i["iterations"] and i["niter"] == list(range(1, i["iterations"] + 1))
