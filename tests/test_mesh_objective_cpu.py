"""CPU suite: mesh objectives compiled at run time (lbfgspp_amd.MeshObjective, lbfgsx_objective_compile_mesh of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mesh_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_mesh_eval", "k_mesh_trial", "k_mesh_b_eval", "k_mesh_b_dg_maxstep_trial")
KD = [(K, D) for K in (2, 3, 4) for D in (1, 2, 3)]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _meshes(K, N):
    return {"strip": MR.strip(K, N), "reversed": MR.reversed_strip(K, N), "fan": MR.fan(K, N, N // 2),
            "random": MR.random_mesh(K, N, 7 + N)}


def _instance(N, D, E, dtype):
    rng = np.random.default_rng(100 * N + E + D)
    return (rng.standard_normal(N * D).astype(dtype), (0.5 + rng.random(E)).astype(dtype), (0.5 + rng.random(N)).astype(dtype),
            rng.standard_normal(N * D).astype(dtype))


# ---------------------------------------------------------------- the reference module's self-checks
@pytest.mark.parametrize("K", [2, 3, 4])
def test_incidence_lists_every_element_K_times_in_ascending_element_order(K):
    for N in (K, K + 1, 7, 12):
        for name, el in _meshes(K, N).items():
            E = el.shape[0]
            assert el.shape[1] == K and el.min() >= 0 and el.max() < N, name
            assert all(len(set(row)) == K for row in el.tolist()), name
            off, words = MR.incidence(el, N)
            assert off.dtype == np.uint32 and words.dtype == np.uint32 and words.shape == (K * E, K)
            assert off[0] == 0 and off[N] == K * E and (np.diff(off.astype(np.int64)) >= 0).all()
            es = words[:, 0].astype(np.int64)
            assert sorted(((es >> 2) * K + (es & 3)).tolist()) == list(range(K * E))  # every (e, slot) once
            for v in range(N):
                mine = es[off[v]:off[v + 1]]
                assert (np.diff(mine >> 2) > 0).all()  # ascending e: a node has one slot of an element
                for q in range(int(off[v]), int(off[v + 1])):
                    e, slot = int(es[q]) >> 2, int(es[q]) & 3
                    assert el[e, slot] == v and words[q, 1:].tolist() == [el[e, k] for k in range(K) if k != slot]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K,D", [(2, 1), (3, 2), (4, 3)])
def test_mesh_grad_is_the_triple_loop_bit_for_bit(K, D, dtype):
    for N in (K, K + 1, 7, 12):
        for name, el in _meshes(K, N).items():
            x, p0, p1, p2 = _instance(N, D, el.shape[0], dtype)
            tg, v = MR.asym_elem_terms(x, el, D, p0, p1)
            ng, nv = MR.node_terms(x, D, p2)
            assert v.dtype == dtype and nv.dtype == dtype and tg.dtype == dtype and ng.dtype == dtype
            for node_g in (None, ng):
                g = MR.mesh_grad(tg, el, N, node_g)
                assert g.dtype == dtype and g.shape == (N * D,)
                assert g.tobytes() == MR.mesh_grad_scalar(tg, el, N, node_g).tobytes(), (name, N)


def test_an_isolated_node_gets_plus_zero():
    el = np.array([[0, 3, 5], [5, 0, 3]])
    x, p0, p1, _ = _instance(6, 2, 2, np.float64)
    g = MR.mesh_grad(MR.asym_elem_terms(x, el, 2, p0, p1)[0], el, 6).reshape(6, 2)
    assert g[[1, 2, 4]].tobytes() == np.zeros((3, 2)).tobytes() and (g[[0, 3, 5]] != 0).all()


def _asym_elem_scalar(dt, K, D, xs, p0e, p1s, e, scalars=MR.SCALARS):
    """one element of ASYM_ELEM in scalar arithmetic of dtype dt, operation for operation"""
    s = dt(0)
    for k in range(K):
        for d in range(D):
            s = dt(s + dt(dt(dt(k * D + d + 1) * p1s[k]) * xs[k * D + d]))
    q = dt(dt(p0e * s) + dt(dt(dt(e) * dt(scalars[0])) + dt(scalars[1])))
    pq = dt(p0e * q)
    return [dt(dt(dt(k * D + d + 1) * p1s[k]) * pq) for k in range(K) for d in range(D)], dt(dt(0.5) * dt(q * q))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K,D", [(2, 3), (3, 2), (4, 3)])
def test_the_restatement_is_the_scalar_statement_and_a_swap_changes_the_bits(K, D, dtype):
    N = 9
    el = MR.random_mesh(K, N, 3)
    x, p0, p1, _ = _instance(N, D, el.shape[0], dtype)
    dt = np.dtype(dtype).type
    tg, v = MR.asym_elem_terms(x, el, D, p0, p1)
    for e in range(el.shape[0]):
        xs = x.reshape(N, D)[el[e]].reshape(-1)
        g, val = _asym_elem_scalar(dt, K, D, xs, p0[e], p1[el[e]], e)
        assert val.tobytes() == v[e].tobytes() and [a.tobytes() for a in g] == [a.tobytes() for a in tg[e].reshape(-1)]
    # a swapped slot, a swapped unknown or a wrong e changes the value
    e = 4
    xs, ps = x.reshape(N, D)[el[e]], p1[el[e]]
    good = _asym_elem_scalar(dt, K, D, xs.reshape(-1), p0[e], ps, e)[1]
    assert _asym_elem_scalar(dt, K, D, xs[::-1].reshape(-1), p0[e], ps[::-1], e)[1] != good
    if D > 1:
        assert _asym_elem_scalar(dt, K, D, xs[:, ::-1].reshape(-1), p0[e], ps, e)[1] != good
    assert _asym_elem_scalar(dt, K, D, xs.reshape(-1), p0[e], ps, e + 1)[1] != good


def _fd_check(f_terms, grad, x, tol):
    for j in range(x.size):
        h = np.zeros(x.size)
        h[j] = 1e-6
        fd = (f_terms(x + h) - f_terms(x - h)) / 2e-6
        assert abs(fd - grad[j]) <= tol * (1.0 + abs(grad[j])), (j, fd, grad[j])


def _total(*terms):
    return float(sum(Fraction(float(t)) for part in terms for t in part))


def test_the_gradients_are_the_derivatives():
    rng = np.random.default_rng(1)
    for K, D in ((2, 1), (3, 2), (4, 3)):
        N = 8
        el = MR.random_mesh(K, N, 2)
        x, p0, p1, p2 = _instance(N, D, el.shape[0], np.float64)
        grad = MR.mesh_grad(MR.asym_elem_terms(x, el, D, p0, p1)[0], el, N, MR.node_terms(x, D, p2)[0])
        _fd_check(lambda y: _total(MR.asym_elem_terms(y, el, D, p0, p1)[1], MR.node_terms(y, D, p2)[1]), grad, x, 1e-6)
        grad = MR.mesh_grad(MR.pairs_terms(x, el, D, p0)[0], el, N, MR.fidelity_terms(x, D, p2)[0])
        _fd_check(lambda y: _total(MR.pairs_terms(y, el, D, p0)[1], MR.fidelity_terms(y, D, p2)[1]), grad, x, 1e-6)
    el = MR.strip(3, 9)
    x, p0 = rng.standard_normal(9), 0.5 + rng.random(9)
    _fd_check(lambda y: _total(MR.triple_terms(y, el, p0)[1]), MR.mesh_grad(MR.triple_terms(x, el, p0)[0], el, 9), x, 1e-5)
    tri, pos = MR.lattice(3, (3, 4))
    x = (pos + 0.1 * rng.standard_normal(pos.shape)).reshape(-1)
    l = [1.0 + 0.1 * rng.random(tri.shape[0]) for _ in range(3)]
    grad = MR.mesh_grad(MR.triangle_terms(x, tri, *l, 0.7, 1.0)[0], tri, 12, MR.tie_terms(x, 2, pos.reshape(-1), 0.3)[0])
    _fd_check(lambda y: _total(MR.triangle_terms(y, tri, *l, 0.7, 1.0)[1], MR.tie_terms(y, 2, pos.reshape(-1), 0.3)[1]), grad, x, 1e-5)
    tet, pos = MR.lattice(4, (2, 3, 2))
    x = (pos + 0.1 * rng.standard_normal(pos.shape)).reshape(-1)
    p0 = np.ones(tet.shape[0])
    _fd_check(lambda y: _total(MR.volume_terms(y, tet, p0)[1]), MR.mesh_grad(MR.volume_terms(x, tet, p0)[0], tet, 12), x, 1e-5)


def test_trial_depth_table_is_the_headers():
    src = open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "mesh_kernels.cuh")).read()
    assert "static constexpr int value = (D == 1) ? 2 : 1;" in src and MR.TRIAL_U == {1: 2, 2: 1, 3: 1}


# ---------------------------------------------------------------- compilation
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K,D", KD)
def test_every_body_compiles_for_every_K_D_and_dtype_without_scratch(A, K, D, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    bodies = list(MR.GENERIC_BODIES)
    if (K, D) == (3, 1):
        bodies.append(("triple", MR.ALIAS_I + MR.TRIPLE, None))
    if (K, D) == (3, 2):
        bodies.append(("triangle", MR.TRIANGLE, MR.TIE_NODE))
    if (K, D) == (4, 3):
        bodies.append(("volume", MR.VOLUME, None))
    for name, elem, node in bodies:
        f = A.MeshObjective(elem, MR.strip(K, K), D, node_body=node)
        info = f.info(dtype)
        print("K %d D %d %s %s: vgprs %d scratch %s" % (K, D, np.dtype(dtype).name, name, info["vgprs"], info["scratch_by_kernel"]))
        assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values()), name
        assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
        h = f.compile(dtype)
        assert core.lbfgsx_objective_K(h) == K and core.lbfgsx_objective_dim(h) == D and core.lbfgsx_objective_form(h) == 4
        assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_both_bodies_once_and_the_mesh_kernels(A):
    for dtype in (np.float64, np.float32):
        src = A.MeshObjective(MR.ASYM_ELEM, MR.strip(3, 3), 2, node_body=MR.NODE).source(dtype)
        assert src.count(MR.ASYM_ELEM) == 1 and src.count(MR.NODE) == 1
        assert '#line 1 "elem_body"' in src and '#line 1 "node_body"' in src and "kNode = true" in src
        assert '#include "mesh_kernels.cuh"' in src and "const uint32_t* inc;" in src and "const uint32_t* off;" in src
        assert "static constexpr int K = 3;" in src and "static constexpr int D = 2;" in src
        assert "elem(const T (&x)[K * D], T (&g)[K * D], int64_t e, const int64_t (&v)[K])" in src
        assert "node(const T (&x)[D], T (&g)[D], int64_t i)" in src
        for k in KERNELS:
            assert "template __global__ void %s<S, ObjMesh>" % k in src
        assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
        assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    for node in (None, ""):
        src = A.MeshObjective(MR.ASYM_ELEM, MR.strip(3, 3), 2, node_body=node).source()
        assert "kNode = false" in src and '"node_body"' not in src and src.count(MR.ASYM_ELEM) == 1


def test_the_cache_is_keyed_by_form_both_bodies_K_D_and_dtype(A):
    core, _ = A.load()
    elem = "g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];\n// cache test of the mesh form"
    node = "g[0] = x[0]; return T(0.5) * (x[0] * x[0]);\n// cache test of the mesh form"
    graph, mesh = A.GraphObjective(elem, edges=(np.array([0]), np.array([1]))), A.MeshObjective(elem, MR.strip(2, 2), 1)
    ig, im = graph.info(), mesh.info()
    assert not ig["cache_hit"] and not im["cache_hit"]
    hg, hm = graph.compile(), mesh.compile()
    assert hg.value != hm.value and core.lbfgsx_objective_form(hg) == 3 and core.lbfgsx_objective_form(hm) == 4
    assert core.lbfgsx_objective_dim(hg) == 1 and core.lbfgsx_objective_dim(hm) == 1  # D, and 1 for the other forms
    again = A.MeshObjective(elem, MR.fan(2, 9, 4), 1).info()  # the elements are not part of the key
    assert again["cache_hit"] and again["compile_ms"] == im["compile_ms"] and again["vgprs"] == im["vgprs"]
    assert not A.MeshObjective(elem, MR.strip(2, 2), 1, node_body=node).info()["cache_hit"]  # the node body is
    assert A.MeshObjective(elem, MR.strip(2, 2), 1, node_body=node).info()["cache_hit"]
    assert not A.MeshObjective(elem, MR.strip(2, 2), 2).info()["cache_hit"]  # D is
    assert not A.MeshObjective(elem, MR.strip(3, 3), 1).info()["cache_hit"]  # K is
    assert not A.MeshObjective(elem, MR.strip(2, 2), 1).info(np.float32)["cache_hit"]


# ---------------------------------------------------------------- refusals
def test_refused_requests_name_the_value(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    bad = "%s volatile(\"\");\ng[0] = g[1] = x[0];\nreturn x[0];" % word
    with pytest.raises(ValueError, match="the element body contains .* inline assembly is not accepted"):
        A.MeshObjective(bad, MR.strip(2, 2), 1).compile()
    with pytest.raises(ValueError, match="the node body contains .* inline assembly is not accepted"):
        A.MeshObjective(MR.PAIRS_ELEM, MR.strip(2, 2), 1, node_body="g[0] = x[0]; __%s__(\"\"); return x[0];" % word).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    body = MR.PAIRS_ELEM.encode()
    assert core.lbfgsx_objective_compile_mesh(C.byref(h), L.F64, 3, 2, None, b"", log, len(log)) == L.E_INVALID
    assert not h.value and b"mesh objective: empty element body" in log.value
    assert core.lbfgsx_objective_source_mesh(L.F64, 3, 2, None, b"", None, 0) == L.E_INVALID
    for K, D, what in ((1, 2, b"K = 1 is not supported"), (5, 2, b"K = 5 is not supported"), (3, 0, b"D = 0 is not supported"),
                       (3, 4, b"D = 4 is not supported")):
        assert core.lbfgsx_objective_compile_mesh(C.byref(h), L.F64, K, D, None, body, log, len(log)) == L.E_INVALID
        assert what in log.value and not h.value
        assert core.lbfgsx_objective_source_mesh(L.F64, K, D, None, body, None, 0) == L.E_INVALID
    assert core.lbfgsx_objective_compile_mesh(C.byref(h), 7, 3, 2, None, body, log, len(log)) == L.E_INVALID
    assert b"unknown dtype" in log.value


def test_compile_errors_name_the_body_and_its_line(A):
    bad_elem = "const T d = x[0] - x[1];\ng[0] = d;\ng[1] = T(0) - d\nreturn d * d;"  # line 3 lacks its semicolon
    bad_node = "const T r = x[0]\ng[0] = r;\nreturn r * r;"                           # line 1 does
    with pytest.raises(ValueError) as e:
        A.MeshObjective(bad_elem, MR.strip(2, 2), 1, node_body=MR.NODE).compile()
    assert "MeshObjective" in str(e.value) and "elem_body:3:" in str(e.value) and "node_body:" not in str(e.value)
    with pytest.raises(ValueError) as e:
        A.MeshObjective(MR.PAIRS_ELEM, MR.strip(2, 2), 1, node_body=bad_node).compile()
    assert "node_body:1:" in str(e.value) and "elem_body:" not in str(e.value) and "error" in str(e.value)


def test_python_side_value_errors(A):
    with pytest.raises(ValueError, match="not one of shape \\(6,\\)"):
        A.MeshObjective(MR.PAIRS_ELEM, np.arange(6), 2)
    with pytest.raises(ValueError, match="K = 5 is not supported"):
        A.MeshObjective(MR.PAIRS_ELEM, np.arange(10).reshape(2, 5), 2)
    with pytest.raises(ValueError, match="not one of dtype float64"):
        A.MeshObjective(MR.PAIRS_ELEM, np.array([[0.0, 1.0, 2.0]]), 2)
    with pytest.raises(ValueError, match="elements holds 4294967296, which does not fit a 32-bit node index"):
        A.MeshObjective(MR.PAIRS_ELEM, np.array([[0, 1, 2 ** 32]]), 2)
    with pytest.raises(ValueError, match="elements holds -2147483649"):
        A.MeshObjective(MR.PAIRS_ELEM, np.array([[0, 1, -2 ** 31 - 1]]), 2)
    with pytest.raises(ValueError, match="E = 0"):
        A.MeshObjective(MR.PAIRS_ELEM, np.zeros((0, 3), np.int64), 2)
    with pytest.raises(ValueError, match="dim = 4 is not supported"):
        A.MeshObjective(MR.PAIRS_ELEM, MR.strip(3, 3), 4)
    with pytest.raises(ValueError, match="MeshObjective: 5 data arrays given, at most 4"):
        A.MeshObjective(MR.PAIRS_ELEM, MR.strip(3, 3), 2, data=[np.ones(3)] * 5)
    f = A.MeshObjective(MR.PAIRS_ELEM, np.array([[0, 1, 2], [2, 1, 3]], np.uint8), 2)
    assert f.elements.dtype == np.int32 and (f.E, f.K, f.D) == (2, 3, 2) and f.elements.tolist() == [[0, 1, 2], [2, 1, 3]]
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="n = 7 is not a multiple of D = 2"):
        s.minimize(f, np.zeros(7))
    f.set_data(np.ones(7))  # n = 8, N = 4 and E = 2: none of them
    with pytest.raises(ValueError, match="MeshObjective: data\\[0\\] must have 8 or 4 or 2 elements"):
        s.minimize(f, np.zeros(8))


def test_the_solver_entry_points_refuse_by_form_before_a_device_is_needed(A):
    from lbfgspp_amd import _lib as L
    _, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    fm = A.MeshObjective(MR.PAIRS_ELEM, MR.strip(3, 4), 2)  # the handles live as long as their objects
    fg = A.GraphObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", edges=(np.array([0]), np.array([1])))
    hm, hg = fm.compile(), fg.compile()
    x = np.zeros(8)
    xp = x.ctypes.data_as(C.c_void_p)
    el = fm.elements.ctypes.data_as(C.POINTER(C.c_int32))
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hm, 8, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"lbfgsx_solver_minimize_mesh" in res.msg
    rc = sol.lbfgsx_solver_minimize_graph(s._h, hm, 8, 2, el, el, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"mesh objective" in res.msg and b"lbfgsx_solver_minimize_mesh" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, hg, 8, 2, el, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a mesh objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, hm, 8, 0, el, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"E = 0" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, hm, 7, 2, el, 0, None, 0, None, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"n = 7 is not a multiple of D = 2" in res.msg
    rc = sol.lbfgsx_solver_minimize_mesh(s._h, fm.compile(np.float32), 8, 2, el, 0, None, 0, None, None, xp, None, None, None,
                                         C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg


NEW_CORE = ["lbfgsx_objective_compile_mesh", "lbfgsx_objective_source_mesh", "lbfgsx_objective_bind_mesh",
            "lbfgsx_objective_mesh_topology", "lbfgsx_objective_dim"]
NEW_SOLVER = ["lbfgsx_solver_minimize_mesh"]


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
    assert "LBFGSX_FORM_GRAPH = 3" in text and re.search(r"LBFGSX_FORM_MESH = 4\b", text)
    assert "MeshObjective" in A.__all__


def test_the_probe_compiles_against_include_as_a_device_build(tmp_path):
    """tests/cpp/mesh_probe.cpp with MeshObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "mesh_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DMESH_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "mesh_probe.cpp"),
           "-L", lib, "-llbfgsx", "-Wl,-rpath," + lib, "-o", exe]
    subprocess.run(cmd, check=True)
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "mesh_probe.cpp")).read()
    for body in (MR.TRIANGLE, MR.TIE_NODE):  # the probe holds the two bodies line by line
        for line in body.splitlines():
            assert '"%s' % line in src, line
