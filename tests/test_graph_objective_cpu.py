"""CPU suite: graph objectives compiled at run time (lbfgspp_amd.GraphObjective, lbfgsx_objective_compile_graph of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import graph_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_graph_eval", "k_graph_trial", "k_graph_b_eval", "k_graph_b_dg_maxstep_trial")


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _graphs(n):
    return {"path": GR.path(n), "reversed": GR.reversed_path(n), "star": GR.star(n, n // 2), "random": GR.random_multigraph(n, 7 + n),
            "ring": GR.ring_chords(n)}


def _instance(n, E, dtype):
    rng = np.random.default_rng(100 * n + E)
    return (rng.standard_normal(n).astype(dtype), (0.5 + rng.random(E)).astype(dtype), (0.5 + rng.random(n)).astype(dtype))


# ---------------------------------------------------------------- the reference module's self-checks
@pytest.mark.parametrize("n", [2, 3, 7, 12])
def test_incidence_lists_every_edge_twice_in_ascending_edge_order(n):
    for name, (ei, ej) in _graphs(n).items():
        E = ei.size
        assert (ei != ej).all(), name
        off, other, es = GR.incidence(ei, ej, n)
        assert off.dtype == np.uint32 and other.dtype == np.int32 and es.dtype == np.uint32
        assert off[0] == 0 and off[n] == 2 * E and (np.diff(off.astype(np.int64)) >= 0).all()
        assert sorted(es.tolist()) == list(range(2 * E))  # every (e, side) once
        for v in range(n):
            mine = es[off[v]:off[v + 1]].astype(np.int64)
            assert (np.diff(mine >> 1) > 0).all()  # ascending e: a node is one end of an edge, not both
            for q in range(int(off[v]), int(off[v + 1])):
                e, side = int(es[q]) >> 1, int(es[q]) & 1
                assert (ei[e], ej[e])[side] == v and (ei[e], ej[e])[1 - side] == other[q]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 7, 12])
def test_graph_grad_is_the_double_loop_bit_for_bit(n, dtype):
    for name, (ei, ej) in _graphs(n).items():
        x, p0, p1 = _instance(n, ei.size, dtype)
        tg, v = GR.asym_edge_terms(x, ei, ej, p0, p1)
        ng, nv = GR.node_terms(x, p1)
        assert v.dtype == dtype and nv.dtype == dtype and all(a.dtype == dtype for a in tg) and ng.dtype == dtype
        for node_g in (None, ng):
            g = GR.graph_grad(tg, ei, ej, n, node_g)
            assert g.dtype == dtype and g.tobytes() == GR.graph_grad_scalar(tg, ei, ej, n, node_g).tobytes(), name


def test_an_isolated_node_gets_plus_zero():
    ei, ej = np.array([0, 3]), np.array([3, 0])
    x, p0, p1 = _instance(5, 2, np.float64)
    g = GR.graph_grad(GR.asym_edge_terms(x, ei, ej, p0, p1)[0], ei, ej, 5)
    assert g[[1, 2, 4]].tobytes() == np.zeros(3).tobytes() and g[0] != 0 and g[3] != 0


def _asym_edge_scalar(dt, x0, x1, we, wi, wj, e, scalars=GR.SCALARS):
    """one edge of ASYM_EDGE in scalar arithmetic of dtype dt, operation for operation"""
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    a = dt(we * wi)
    s = dt(dt(a * x0) + dt(dt(2) * dt(wj * x1)))
    q = dt(s + dt(dt(dt(e) * c0) + c1))
    return [dt(a * q), dt(dt(2) * dt(wj * q))], dt(dt(0.5) * dt(q * q))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatements_are_the_scalar_statements_and_the_gradient_is_the_derivative(dtype):
    n = 9
    ei, ej = GR.random_multigraph(n, 3)
    x, p0, p1 = _instance(n, ei.size, dtype)
    dt = np.dtype(dtype).type
    tg, v = GR.asym_edge_terms(x, ei, ej, p0, p1)
    for e in range(ei.size):
        g, val = _asym_edge_scalar(dt, x[ei[e]], x[ej[e]], p0[e], p1[ei[e]], p1[ej[e]], e)
        assert val.tobytes() == v[e].tobytes() and [a.tobytes() for a in g] == [tg[0][e].tobytes(), tg[1][e].tobytes()]
    if dtype == np.float64:  # central differences of the sum of the values, in rational arithmetic for the sum itself
        def f(y):
            return float(sum(Fraction(float(t)) for t in GR.asym_edge_terms(y, ei, ej, p0, p1)[1]) +
                         sum(Fraction(float(t)) for t in GR.node_terms(y, p1)[1]))
        grad = GR.graph_grad(tg, ei, ej, n, GR.node_terms(x, p1)[0])
        for j in range(n):
            h = np.zeros(n)
            h[j] = 1e-6
            fd = (f(x + h) - f(x - h)) / 2e-6
            assert abs(fd - grad[j]) <= 1e-6 * (1.0 + abs(grad[j]))
        for name, terms in (("spring", lambda y: GR.spring_terms(y, ei, ej, p0)), ("pair", lambda y: GR.pair_terms(y, ei, ej, p1))):
            grad = GR.graph_grad(terms(x)[0], ei, ej, n)
            for j in range(n):
                h = np.zeros(n)
                h[j] = 1e-6
                fd = (terms(x + h)[1].sum() - terms(x - h)[1].sum()) / 2e-6
                assert abs(fd - grad[j]) <= 1e-5 * (1.0 + abs(grad[j])), name


def test_the_ring_and_chords_graph_is_the_probes():
    ei, ej = GR.ring_chords(96)
    assert ei.size == 96 + 32 and (ei[:3].tolist(), ej[:3].tolist()) == ([0, 3, 1], [1, 0, 2])
    assert (ei != ej).all() and ei.min() == 0 and ei.max() == 95
    assert GR.ring_weights(7).tolist() == [1.0, 1.25, 1.5, 1.75, 2.0, 1.0, 1.25]
    src = open(os.path.join(ROOT, "tests", "cpp", "graph_probe.cpp")).read()
    for body in (GR.SPRING_EDGE, GR.WELL_NODE):  # the probe holds the two bodies line by line
        for line in body.splitlines():
            assert '"%s' % line in src, line


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("node", [None, GR.NODE], ids=["edges", "edges+nodes"])
def test_the_bodies_compile_for_both_dtypes_without_scratch(A, node, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.GraphObjective(GR.ASYM_EDGE, edges=GR.path(3), node_body=node)
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == 2 and core.lbfgsx_objective_form(h) == 3
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_solver_tests_bodies_compile_without_scratch(A, dtype):
    for edge, node in ((GR.SPRING_EDGE, GR.WELL_NODE), (GR.SPRING_EDGE, GR.FIDELITY_NODE), (GR.PAIR, None)):
        info = A.GraphObjective(edge, edges=GR.path(3), node_body=node).info(dtype)
        print(info)
        assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())


def test_generated_source_holds_both_bodies_once_and_the_graph_kernels(A):
    for dtype in (np.float64, np.float32):
        src = A.GraphObjective(GR.ASYM_EDGE, edges=GR.path(3), node_body=GR.NODE).source(dtype)
        assert src.count(GR.ASYM_EDGE) == 1 and src.count(GR.NODE) == 1
        assert '#line 1 "edge_body"' in src and '#line 1 "node_body"' in src and "kNode = true" in src
        assert '#include "graph_kernels.cuh"' in src and "const GraphEntry* inc;" in src and "const uint32_t* off;" in src
        assert "edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j)" in src
        assert "node(const T (&x)[1], T (&g)[1], int64_t i)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjGraph>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    for node in (None, ""):
        src = A.GraphObjective(GR.ASYM_EDGE, edges=GR.path(3), node_body=node).source()
        assert "kNode = false" in src and '"node_body"' not in src and src.count(GR.ASYM_EDGE) == 1


def test_the_cache_is_keyed_by_form_both_bodies_and_dtype(A):
    core, _ = A.load()
    edge = "g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];\n// cache test of the graph form"
    node = "g[0] = x[0]; return T(0.5) * (x[0] * x[0]);\n// cache test of the graph form"
    chain, graph = A.ChainObjective(edge, K=2), A.GraphObjective(edge, edges=GR.path(2))
    ic, ig = chain.info(), graph.info()
    assert not ic["cache_hit"] and not ig["cache_hit"]
    hc, hg = chain.compile(), graph.compile()
    assert hc.value != hg.value and core.lbfgsx_objective_form(hc) == 1 and core.lbfgsx_objective_form(hg) == 3
    again = A.GraphObjective(edge, edges=GR.star(9, 4)).info()  # the edges are not part of the key
    assert again["cache_hit"] and again["compile_ms"] == ig["compile_ms"] and again["vgprs"] == ig["vgprs"]
    assert not A.GraphObjective(edge, edges=GR.path(2), node_body=node).info()["cache_hit"]  # the node body is
    assert A.GraphObjective(edge, edges=GR.path(2), node_body=node).info()["cache_hit"]
    assert not A.GraphObjective(edge, edges=GR.path(2)).info(np.float32)["cache_hit"]


# ---------------------------------------------------------------- refusals
def test_a_body_with_inline_assembly_or_no_edge_body_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    bad = "%s volatile(\"\");\ng[0] = g[1] = x[0];\nreturn x[0];" % word
    with pytest.raises(ValueError, match="the edge body contains .* inline assembly is not accepted"):
        A.GraphObjective(bad, edges=GR.path(2)).compile()
    with pytest.raises(ValueError, match="the node body contains .* inline assembly is not accepted"):
        A.GraphObjective(GR.SPRING_EDGE, edges=GR.path(2), node_body="g[0] = x[0]; __%s__(\"\"); return x[0];" % word).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    assert core.lbfgsx_objective_compile_graph(C.byref(h), L.F64, None, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"graph objective: empty edge body" in log.value
    assert core.lbfgsx_objective_source_graph(L.F64, None, b"", None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_graph(C.byref(h), 7, None, GR.SPRING_EDGE.encode(), log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


def test_compile_errors_name_the_body_and_its_line(A):
    bad_edge = "const T d = x[0] - x[1];\ng[0] = d;\ng[1] = T(0) - d\nreturn d * d;"  # line 3 lacks its semicolon
    bad_node = "const T r = x[0]\ng[0] = r;\nreturn r * r;"                           # line 1 does
    with pytest.raises(ValueError) as e:
        A.GraphObjective(bad_edge, edges=GR.path(2), node_body=GR.NODE).compile()
    assert "GraphObjective" in str(e.value) and "edge_body:3:" in str(e.value) and "node_body:" not in str(e.value)
    with pytest.raises(ValueError) as e:
        A.GraphObjective(GR.SPRING_EDGE, edges=GR.path(2), node_body=bad_node).compile()
    assert "node_body:1:" in str(e.value) and "edge_body:" not in str(e.value) and "error" in str(e.value)


def test_python_side_value_errors(A):
    with pytest.raises(ValueError, match="ei has 3 elements and ej has 2"):
        A.GraphObjective(GR.SPRING_EDGE, edges=(np.arange(3), np.arange(2)))
    with pytest.raises(ValueError, match="E = 0"):
        A.GraphObjective(GR.SPRING_EDGE, edges=(np.zeros(0, np.int64), np.zeros(0, np.int64)))
    with pytest.raises(ValueError, match="ej holds 4294967296, which does not fit a 32-bit node index"):
        A.GraphObjective(GR.SPRING_EDGE, edges=(np.array([0, 1]), np.array([1, 2 ** 32])))
    with pytest.raises(ValueError, match="ei holds -2147483649"):
        A.GraphObjective(GR.SPRING_EDGE, edges=(np.array([-2 ** 31 - 1, 1]), np.array([1, 2])))
    with pytest.raises(ValueError, match="ei must be a 1-D integer array"):
        A.GraphObjective(GR.SPRING_EDGE, edges=(np.array([0.0, 1.0]), np.array([1, 2])))
    with pytest.raises(ValueError, match="edges must be a pair"):
        A.GraphObjective(GR.SPRING_EDGE, edges=np.arange(3))
    with pytest.raises(ValueError, match="GraphObjective: 5 data arrays given, at most 4"):
        A.GraphObjective(GR.SPRING_EDGE, edges=GR.path(3), data=[np.ones(3)] * 5)
    f = A.GraphObjective(GR.SPRING_EDGE, edges=(np.array([0, 1, 2, 0], np.uint8), np.array([1, 2, 3, 2], np.int16)))
    assert f.ei.dtype == np.int32 and f.ej.dtype == np.int32 and f.E == 4 and f.ej.tolist() == [1, 2, 3, 2]
    s = A.LBFGSSolver(A.LBFGSParam())
    f.set_data(np.ones(7))  # n = 6 and E = 4: neither
    with pytest.raises(ValueError, match="GraphObjective: data\\[0\\] must have 6 or 4 elements"):
        s.minimize(f, np.zeros(6))


def test_the_solver_entry_points_refuse_by_form_before_a_device_is_needed(A):
    from lbfgspp_amd import _lib as L
    _, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    fg = A.GraphObjective(GR.SPRING_EDGE, edges=GR.path(3))  # the handles live as long as their objects
    fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
    hg, hc = fg.compile(), fc.compile()
    x = np.zeros(6)
    xp = x.ctypes.data_as(C.c_void_p)
    ei, ej = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in (fg.ei, fg.ej))
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hg, 6, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"lbfgsx_solver_minimize_graph" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, hc, 6, 2, ei, ej, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a graph objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, hg, 6, 0, ei, ej, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"E = 0" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, fg.compile(np.float32), 6, 2, ei, ej, 0, None, 0, None, None, xp, None, None, None,
                                          C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg


NEW_CORE = ["lbfgsx_objective_compile_graph", "lbfgsx_objective_source_graph", "lbfgsx_objective_bind_graph",
            "lbfgsx_objective_topology", "lbfgsx_objective_upload_count"]
NEW_SOLVER = ["lbfgsx_solver_minimize_graph"]


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
    assert "LBFGSX_FORM_GRAPH = 3" in open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    assert "GraphObjective" in A.__all__


def test_the_probe_compiles_against_include_as_a_device_build(tmp_path):
    """tests/cpp/graph_probe.cpp with GraphObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "graph_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DGRAPH_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "graph_probe.cpp"),
           "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o", exe]
    subprocess.run(cmd, check=True)
    assert os.path.exists(exe)
