"""CPU suite: graph-regularised linear-model objectives compiled at run time (lbfgspp_amd.GraphLinearObjective,
lbfgsx_objective_compile_linear_graph of include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed
target gfx950, what the code object says about its kernels is read from the code object itself, and the numpy restatement
(tests/graph_linear_ref.py) is checked against exact rational arithmetic and against its own plain-loop form."""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import graph_linear_ref as GL
import graph_ref as GR
import linear_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_ling_eval", "k_ling_trial", "k_ling_b_eval", "k_ling_b_dg_maxstep_trial", "k_lin_rows", "k_lin_rows_trial")
M2 = (np.array([0, 2]), np.array([1, 0]), np.array([1.0, -0.5]))  # the 1 x 2 matrix
E2 = (np.array([1]), np.array([0]))                               # its one edge
FORM = 8


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _obj(A, row=LR.HINGE, edge=GL.SPRING_EDGE, coord=None, **kw):
    return A.GraphLinearObjective(row, M2, E2, edge, n=2, coord_body=coord, **kw)


# ---------------------------------------------------------------- the reference module's self-checks
def _gamma(k, dt):
    u = float(np.finfo(dt).eps) / 2
    return Fraction(k * u) / (1 - Fraction(k * u))


def _instances(dtype):
    big = GL.Problem(LR.long_columns(dtype, R=700, n=9, C=256), *GR.star(9, 0))
    return (GL.pair(dtype), GL.tiny(dtype), GL.Problem(LR.random_rows(60, 23, 40, 9, dtype), *GR.random_multigraph(23, 5)), big)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_agrees_with_exact_sums_within_the_bound_of_its_lengths(dtype):
    """With the restatement's own w and edge partials taken as exact inputs, grad[j] is psi' plus deg_j edge partials plus len_j
    rounded products, summed through at most deg_j + len_j rounded additions in SOME order (chunk partials are just another
    order): |grad[j] - exact| <= gamma(deg_j + len_j + 1) * (|psi'| + sum |g_e| + sum |val w|), gamma(k) = k u / (1 - k u)
    (Higham, Accuracy and Stability, section 3.1).  The vectorised form equals the plain-loop form bit for bit."""
    fr = lambda a: [Fraction(float(v)) for v in a]
    for Q in _instances(dtype):
        P = Q.P
        x = np.random.default_rng(4).standard_normal(Q.n).astype(dtype)
        w, _ = LR.cubic(P.z(x, 8), P.p0)
        pg, _ = LR.ridge(x, P.c0)
        colptr, trow, tpos = P.topo
        fval, fw = fr(P.val), fr(w)
        for edge in ("asym", "spring"):
            tg, _ = GL.edge_terms(edge, x, Q.ei.astype(np.int64), Q.ej.astype(np.int64), Q.p2, Q.p3)
            ftg = [fr(tg[0]), fr(tg[1])]
            for psi in (None, pg):
                g = GL.gradient(w, P.val, P.topo, Q.ei, Q.ej, Q.n, tg, P.C, psi)
                gs = GL.gradient_scalar(w, P.val, P.topo, Q.ei, Q.ej, Q.n, tg, P.C, psi)
                assert g.dtype == np.dtype(dtype) and g.tobytes() == gs.tobytes()
                for j in range(Q.n):
                    terms = [Fraction(float(psi[j]))] if psi is not None else []
                    terms += [ftg[s][e] for e in range(Q.E) for s, end in ((0, Q.ei[e]), (1, Q.ej[e])) if end == j]
                    terms += [fval[tpos[q]] * fw[trow[q]] for q in range(colptr[j], colptr[j + 1])]
                    bound = _gamma(len(terms), dtype) * sum((abs(t) for t in terms), Fraction(0))
                    assert abs(Fraction(float(g[j])) - sum(terms, Fraction(0))) <= bound, j
                    if not terms:
                        assert g[j] == 0 and not np.signbit(g[j])
        # without edges at a node and without psi the rule is the linear form's; without a matrix contribution the graph form's
        tg, _ = GL.edge_terms("asym", x, Q.ei.astype(np.int64), Q.ej.astype(np.int64), Q.p2, Q.p3)
        zero_w = np.zeros_like(w)
        only_graph = GL.gradient(zero_w, P.val, P.topo, Q.ei, Q.ej, Q.n, [tg[0], tg[1]], P.C)
        ref = GR.graph_grad_scalar(tg, Q.ei, Q.ej, Q.n)
        lens = np.diff(colptr.astype(np.int64))
        assert only_graph[lens == 0].tobytes() == ref[lens == 0].tobytes()


def test_a_coordinate_with_nothing_gets_plus_zero_and_a_sum_starts_from_its_first_contribution():
    dt = np.float64
    Q = GL.tiny(dt)
    off, _, _ = GR.incidence(Q.ei, Q.ej, Q.n)
    lens = np.diff(Q.P.topo[0].astype(np.int64))
    assert np.diff(off.astype(np.int64)).tolist() == [3, 1, 0, 3, 1] and lens.tolist() == [2, 1, 0, 2, 1]  # node 2: nothing
    x = np.random.default_rng(3).standard_normal(Q.n)
    g, terms = Q.evaluate(x, 1, "cubic", "asym", False)
    assert g[2] == 0 and not np.signbit(g[2])
    assert terms.size == Q.E + Q.R
    g, terms = Q.evaluate(x, 1, "cubic", "asym", True)
    assert g[2] == LR.ridge(x, Q.P.c0)[0][2] and terms.size == Q.n + Q.E + Q.R
    # no leading 0 +: a first contribution of -0 stays -0, from an edge ..
    topo = LR.transpose(np.array([0, 1]), np.array([0]), 3)
    ei, ej = np.array([1]), np.array([2])
    tg = [np.array([-0.0]), np.array([0.0])]
    g = GL.gradient(np.array([0.0]), np.array([-1.0]), topo, ei, ej, 3, tg)
    assert np.signbit(g[0]) and g[0] == 0      # column 0: the product -1 * 0 = -0 is its first contribution
    assert np.signbit(g[1]) and g[1] == 0      # node 1: the edge's -0 is its first contribution
    assert not np.signbit(g[2]) and g[2] == 0  # node 2: the edge's +0
    # .. and the edge comes before the column: -0 (edge) + +0 (column) = +0, where the column alone would give -0
    tg = [np.array([0.0]), np.array([0.0])]
    g = GL.gradient(np.array([0.0]), np.array([-1.0]), LR.transpose(np.array([0, 1]), np.array([1]), 3), ei, ej, 3, tg)
    assert not np.signbit(g[1]) and g[1] == 0
    # the order is psi, edges, column: (a + b) + c with a = 1, b = 2^-53, c = 2^-53 rounds b away twice
    u = 2.0 ** -53
    g = GL.gradient(np.array([1.0]), np.array([u]), LR.transpose(np.array([0, 1]), np.array([1]), 3), ei, ej, 3,
                    [np.array([u]), np.array([0.0])], psi_g=np.array([0.0, 1.0, 0.0]))
    assert g[1] == 1.0
    g = GL.gradient(np.array([1.0]), np.array([1.0]), LR.transpose(np.array([0, 1]), np.array([1]), 3), ei, ej, 3,
                    [np.array([u]), np.array([0.0])], psi_g=np.array([0.0, u, 0.0]))
    assert g[1] == 1.0 + 2 * u  # (u + u) + 1 is exact: the small ones met first


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_both_dtypes_compile_with_zero_scratch_in_all_six_kernels(A, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    most = 0
    # every body of the GPU tests and the logistic row body of the measurements, each edge body with and without a coordinate body
    for name, row, ename, coord in (("cubic", LR.CUBIC, "asym", LR.RIDGE), ("hinge", LR.HINGE, "asym", None),
                                    ("hinge", LR.HINGE, "spring", LR.RIDGE), ("logistic", LR.LOGISTIC, "spring", None)):
        f = _obj(A, row, GL.EDGE_BODIES[ename], coord)
        info = f.info(dtype)
        print("%s %s %s ridge %s: vgprs %d scratch %d" % (np.dtype(dtype).name, name, ename, coord is not None, info["vgprs"],
                                                          info["scratch_bytes"]))
        # the two maxima cover the row passes as well as the four column-pass kernels
        assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values()), name
        assert 0 < info["vgprs"] <= 128 and info["compile_ms"] > 0
        most = max(most, info["vgprs"])
        h = f.compile(dtype)
        assert core.lbfgsx_objective_form(h) == FORM and core.lbfgsx_objective_K(h) == 1
        assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)
    print("largest VGPR count, %s: %d" % (np.dtype(dtype).name, most))


def test_generated_source_names_the_three_bodies_and_the_six_kernels(A):
    for dtype in (np.float64, np.float32):
        src = _obj(A, LR.HINGE, GL.ASYM_EDGE, LR.RIDGE).source(dtype)
        assert src.count(LR.HINGE) == 1 and src.count(LR.RIDGE) == 1 and src.count(GL.ASYM_EDGE) == 1
        for name in ("coord_body", "edge_body", "row_body"):
            assert '#line 1 "%s"' % name in src
        assert src.index('"coord_body"') < src.index('"edge_body"') < src.index('"row_body"') and "kCoord = true" in src
        assert '#include "linear_graph_kernels.cuh"' in src and "struct ObjLinearGraph" in src
        members = src[src.index("T c[8];"):src.index("// the term of coordinate")]
        assert members.index("const int32_t* rowptr;") < members.index("int32_t L, C, nlong, pad_;") \
            < members.index("const uint32_t* off;") < members.index("const GraphEntry* inc;") < members.index("int64_t E;")
        assert "row(const T z, T& dz, int64_t r)" in src and "coord(const T (&x)[1], T (&g)[1], int64_t i)" in src
        assert "edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjLinearGraph>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    for coord in (None, ""):
        src = _obj(A, coord=coord).source()
        assert "kCoord = false" in src and '"coord_body"' not in src and src.count(LR.HINGE) == 1


def test_the_cache_is_keyed_by_form_three_bodies_and_dtype(A):
    row = "dz = z;\nreturn T(0.5) * (z * z);\n// cache test of the graph-regularised form"
    coord = "g[0] = x[0]; return T(0.5) * (x[0] * x[0]);\n// cache test of the graph-regularised form"
    edge = "g[0] = x[1]; g[1] = x[0]; return x[0] * x[1];\n// cache test of the graph-regularised form"
    first = _obj(A, row, edge).info()
    assert not first["cache_hit"]
    Q = GL.tiny(np.float64)
    again = A.GraphLinearObjective(row, (Q.P.rowptr, Q.P.col, Q.P.val), (Q.ei, Q.ej), edge, n=Q.n, lanes=8).info()
    assert again["cache_hit"] and again["compile_ms"] == first["compile_ms"]  # matrix, edges and lanes are not part of the key
    assert not _obj(A, row, edge, coord).info()["cache_hit"] and _obj(A, row, edge, coord).info()["cache_hit"]
    assert not _obj(A, row, edge + " ").info()["cache_hit"]         # the edge body is part of the key
    assert not _obj(A, row + " ", edge).info()["cache_hit"]         # and the row body
    assert not _obj(A, row, edge).info(np.float32)["cache_hit"]
    # the same bodies as a linear-model or as a graph objective are entries of their own
    assert not A.LinearObjective(row, M2, 2, coord_body=coord).info()["cache_hit"]
    assert not A.GraphObjective(edge, E2, node_body=coord).info()["cache_hit"]
    assert _obj(A, row, edge).info()["cache_hit"]


def test_compile_errors_name_the_body_and_its_line(A):
    bad_row = "const T u = z - p0[r];\ndz = u\nreturn u * u;"            # line 2 lacks its semicolon
    bad_coord = "const T q = x[0]\ng[0] = q;\nreturn q * q;"              # line 1 does
    bad_edge = "const T d = x[0] - x[1];\ng[0] = d;\ng[1] = T(0) - d\nreturn d * d;"  # line 3 does
    with pytest.raises(ValueError) as e:
        _obj(A, bad_row, GL.SPRING_EDGE, LR.RIDGE).compile()
    assert "GraphLinearObjective" in str(e.value) and "row_body:2:" in str(e.value)
    assert "coord_body:" not in str(e.value) and "edge_body:" not in str(e.value)
    with pytest.raises(ValueError) as e:
        _obj(A, LR.HINGE, GL.SPRING_EDGE, bad_coord).compile()
    assert "coord_body:1:" in str(e.value) and "row_body:" not in str(e.value) and "edge_body:" not in str(e.value)
    with pytest.raises(ValueError) as e:
        _obj(A, LR.HINGE, bad_edge, LR.RIDGE).compile()
    assert "edge_body:3:" in str(e.value) and "row_body:" not in str(e.value) and "coord_body:" not in str(e.value)


def test_refused_requests_name_the_value(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    with pytest.raises(ValueError, match="the row body contains .* inline assembly is not accepted"):
        _obj(A, "%s volatile(\"\");\ndz = z;\nreturn z;" % word).compile()
    with pytest.raises(ValueError, match="the coordinate body contains .* inline assembly is not accepted"):
        _obj(A, coord="g[0] = x[0]; __%s__(\"\"); return x[0];" % word).compile()
    with pytest.raises(ValueError, match="the edge body contains .* inline assembly is not accepted"):
        _obj(A, edge="g[0] = x[0]; g[1] = x[1]; __%s__(\"\"); return x[0];" % word).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    hinge, spring = LR.HINGE.encode(), GL.SPRING_EDGE.encode()
    assert core.lbfgsx_objective_compile_linear_graph(C.byref(h), L.F64, None, spring, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"graph-regularised linear-model objective: empty row body" in log.value
    for none in (None, b""):
        assert core.lbfgsx_objective_compile_linear_graph(C.byref(h), L.F64, None, none, hinge, log, len(log)) == L.E_INVALID
        assert not h.value and b"graph-regularised linear-model objective: empty edge body" in log.value
        assert core.lbfgsx_objective_source_linear_graph(L.F64, None, none, hinge, None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_linear_graph(C.byref(h), 7, None, spring, hinge, log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


# ---------------------------------------------------------------- the Python class
def test_python_side_value_errors(A):
    rp, col, val = np.array([0, 2, 3]), np.array([0, 1, 1]), np.ones(3)
    m, e = (rp, col, val), (np.array([0]), np.array([1]))
    G = lambda matrix=m, edges=e, n=2, **kw: A.GraphLinearObjective(LR.HINGE, matrix, edges, GL.SPRING_EDGE, n=n, **kw)
    assert issubclass(A.GraphLinearObjective, A.LinearObjective)
    with pytest.raises(ValueError, match="edges must be a pair"):
        G(edges=(np.array([0]),))
    with pytest.raises(ValueError, match="ei must be a 1-D integer array, not float64"):
        G(edges=(np.array([0.0]), np.array([1])))
    with pytest.raises(ValueError, match="ej holds 4294967296, which does not fit a 32-bit node index"):
        G(edges=(np.array([0]), np.array([2 ** 32])))
    with pytest.raises(ValueError, match="ei has 2 elements and ej has 1"):
        G(edges=(np.array([0, 1]), np.array([1])))
    with pytest.raises(ValueError, match="GraphLinearObjective: E = 0"):
        G(edges=(np.zeros(0, int), np.zeros(0, int)))
    with pytest.raises(ValueError, match="n = 1: an edge joins two different coordinates"):
        A.GraphLinearObjective(LR.HINGE, (np.array([0, 1]), np.array([0]), np.ones(1)), e, GL.SPRING_EDGE, n=1)
    with pytest.raises(ValueError, match="matrix must be a triple"):
        G(matrix=(rp, col))
    with pytest.raises(ValueError, match="col has 3 elements and val has 2"):
        G(matrix=(rp, col, np.ones(2)))
    with pytest.raises(ValueError, match="rowptr\\[0\\] = 0 and rowptr\\[R\\] = 2: rowptr starts at 0 and ends at nnz = 3"):
        G(matrix=(np.array([0, 1, 2]), col, val))
    with pytest.raises(ValueError, match="nnz = 0"):
        G(matrix=(np.array([0, 0]), np.zeros(0, int), np.zeros(0)))
    with pytest.raises(ValueError, match="lanes = 3"):
        G(lanes=3)
    with pytest.raises(ValueError, match="GraphLinearObjective: 5 data arrays given, at most 4"):
        G(data=[np.ones(2)] * 5)
    f = G(edges=(np.array([0, 1, 0], np.uint8), [1, 0, 1]), data=(np.ones(2),))
    assert f.ei.dtype == np.int32 and f.ej.dtype == np.int32 and (f.R, f.nnz, f.n, f.E, f.lanes) == (2, 3, 2, 3, 0)
    assert f._data_sizes(2) == (2, 3, 2)
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="the matrix has n = 2 columns and x has 7 elements"):
        s.minimize(f, np.zeros(7))
    f5 = G(data=(np.ones(5),))  # n = 2, E = 1, R = 2: none of them
    with pytest.raises(ValueError, match="GraphLinearObjective: data\\[0\\] must have 2 or 1 or 2 elements"):
        s.minimize(f5, np.zeros(2))


def test_every_entry_point_refuses_by_form_before_a_device_is_needed(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    fc = _obj(A)  # the handles live as long as their objects
    fl = A.LinearObjective(LR.HINGE, M2, 2)
    fg = A.GraphObjective(GL.SPRING_EDGE, E2)
    hc, hl, hg = fc.compile(), fl.compile(), fg.compile()
    x = np.zeros(2)
    xp = x.ctypes.data_as(C.c_void_p)
    rp, cp, vp = (a.ctypes.data_as(C.c_void_p) for a in (np.array([0, 2], np.int32), np.array([1, 0], np.int32), np.ones(2)))
    e0 = np.zeros(1, np.int32)
    e1 = np.ones(1, np.int32)
    i32p = C.POINTER(C.c_int32)
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hc, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"is minimised with its matrix and edges: lbfgsx_solver_minimize_linear_graph" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, hc, 2, 1, e0.ctypes.data_as(i32p), e1.ctypes.data_as(i32p), 0, None, 0, None, None,
                                          xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a graph objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, hc, 2, 1, e0.ctypes.data_as(i32p), 0, None, 0, None, None, xp, None, None, None,
                                         C.byref(res))
    assert rc == L.E_INVALID and b"not a mesh objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_linear(s._h, hc, 2, 1, 2, rp, cp, vp, 0, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a linear-model objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_dense(s._h, hc, 2, 1, vp, 2, 0, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a dense linear-model objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid(s._h, hc, 1, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid objective" in res.msg

    def coupled(h, n=2, R=1, nnz=2, E=1):
        return sol.lbfgsx_solver_minimize_linear_graph(s._h, h, n, R, nnz, rp, cp, vp, 0, 0, E, e0.ctypes.data, e1.ctypes.data, 0,
                                                       None, 0, None, None, xp, None, None, None, C.byref(res))
    for h in (hl, hg):
        assert coupled(h) == L.E_INVALID and b"not a graph-regularised linear-model objective" in res.msg
    assert coupled(hc, E=0) == L.E_INVALID and b"E = 0" in res.msg
    assert coupled(hc, R=0) == L.E_INVALID and b"R = 0, nnz = 2" in res.msg
    assert coupled(hc, nnz=0) == L.E_INVALID and b"R = 1, nnz = 0" in res.msg
    assert coupled(fc.compile(np.float32)) == L.E_INVALID and b"the other dtype" in res.msg


NEW_CORE = ["lbfgsx_objective_compile_linear_graph", "lbfgsx_objective_source_linear_graph", "lbfgsx_objective_bind_linear_graph"]
NEW_SOLVER = ["lbfgsx_solver_minimize_linear_graph"]


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
    assert re.search(r"LBFGSX_FORM_DENSE = 7\b", text) and re.search(r"LBFGSX_FORM_LINEAR_GRAPH = 8\b", text)
    assert "GraphLinearObjective" in A.__all__ and issubclass(A.GraphLinearObjective, A.LinearObjective)


def test_the_cpp_class_compiles_against_include(tmp_path):
    """GraphLinearObjective<Scalar> of include/LBFGSpp/Device.h in both solvers' minimize, built with g++ against include/"""
    src = tmp_path / "graph_linear_use.cpp"
    src.write_text("""#include <vector>
#include <LBFGS.h>
#include <LBFGSB.h>
using namespace LBFGSpp;
static_assert(detail::is_compiled_objective<double, GraphLinearObjective<double> >::value, "registered");
template <class S> S run(const char* row, const char* edge, const char* coord)
{
    std::vector<std::int32_t> rp = {0, 2}, col = {1, 0}, ei = {1}, ej = {0};
    std::vector<S> val = {S(1), S(-0.5)}, y = {S(1)};
    GraphLinearObjective<S> f(row, edge, coord);
    f.matrix(1, 2, rp.data(), col.data(), val.data()).edges(1, ei.data(), ej.data()).host_data(0, y.data(), 1).scalars({0.5});
    Eigen::Matrix<S, Eigen::Dynamic, 1> x = Eigen::Matrix<S, Eigen::Dynamic, 1>::Zero(2), lb = x, ub = x;
    S fx = 0, fb = 0;
    LBFGSParam<S> p;
    LBFGSSolver<S> s(p);
    s.minimize(f, x, fx);
    LBFGSBParam<S> pb;
    LBFGSBSolver<S> sb(pb);
    sb.minimize(f, x, fb, lb, ub);
    return fx + fb;
}
int main(int argc, char** argv)
{
    return argc > 5 ? int(run<double>(argv[1], argv[2], argv[3]) + run<float>(argv[1], argv[2], argv[3])) : 0;
}
""")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "oracle", "eigen_shim"), str(src), "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o",
           str(tmp_path / "graph_linear_use")]
    subprocess.run(cmd, check=True)


def test_the_probe_compiles_against_include_as_a_device_build(tmp_path):
    """tests/cpp/graph_linear_probe.cpp with GraphLinearObjective<double> in place of the functor, built with g++ against
    include/; the fixture it is compared with holds data only"""
    exe = str(tmp_path / "graph_linear_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DGRAPH_LINEAR_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "graph_linear_probe.cpp"),
           "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o", exe]
    subprocess.run(cmd, check=True)
    assert os.path.exists(exe)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "graph_linear_golden.json")))
    assert set(g) == {"tolerance", "constants", "instances"} and g["tolerance"] == 1e-10
    assert sorted((i["solver"], i["R"], i["n"]) for i in g["instances"]) == [("lbfgs", 120, 40), ("lbfgs", 600, 150),
                                                                             ("lbfgsb", 120, 40), ("lbfgsb", 600, 150)]
    for i in g["instances"]:
        assert i["iterations"] >= 8 and len(i["x_f8_base64"]) == i["iterations"] and i["niter"] == list(range(1, i["iterations"] + 1))
