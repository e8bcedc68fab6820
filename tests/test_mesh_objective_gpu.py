"""-m gpu: mesh objectives (lbfgspp_amd.MeshObjective, csrc/mesh_kernels.cuh, csrc/mesh_topology.hip) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/mesh_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal -- on reversed strips, fans and
    random meshes, all bound one after another to one context (the list is rebuilt at every bind);
  * K = 2, D = 1 with a graph's edge body is that GraphObjective bit for bit; the K = 3, D = 1 strip with a chain body is that
    ChainObjective bit for bit;
  * lbfgsx_objective_mesh_topology is the incidence list of the restatement;
  * the triangle energy on the lattice follows the reference (tests/golden/mesh_golden.json), from Python and C++;
  * a convex instance converges to the solution of its linear system under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import graph_ref as GR
import mesh_ref as MR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the nodes a thread owns (the values of a 16-byte pack)


def _node_counts(dtype, K, D, full):
    W = PACK[dtype]
    tile = 256 * MR.TRIAL_U[D]  # node packs
    # K < W at f32 for K = 2 and 3: no whole group of nodes (at f64 W = 2 <= K: there is no smaller mesh); 64 W + 1 has exactly
    # one node past the last group; tile W + 1 is one node past one trial tile
    if not full:
        return [K, 64 * W + 1, tile * W + 1, tile * W + 3]
    # around a wave, a block and one and two trial tiles, with and without tail nodes; about five tiles: several blocks, and
    # both tile orders cross tile borders
    return [K, K + 1, 64 * W - 1, 64 * W + 1, 256 * W + W + 1, tile * W + 1, tile * W + 3, 2 * tile * W + W + 1,
            5 * tile * W + W + 1]


def _shapes():
    out = []
    for dtype in (O.F64, O.F32):
        for K, D, full in ((3, 2, True), (4, 3, True), (2, 1, False), (2, 3, False), (3, 1, False)):
            for N in _node_counts(dtype, K, D, full):
                out.append(pytest.param(dtype, K, D, N, id="%s-K%d-D%d-%d" % ("f64" if dtype == O.F64 else "f32", K, D, N)))
    return out


def _families(K, N):
    """(name, elems, with the node body)"""
    out = [("reversed-strip", MR.reversed_strip(K, N), False)]
    for hub in dict.fromkeys((0, N // 2, N - 1)):  # N - 1 is a tail node when N is no multiple of W
        out.append(("fan-%d" % hub, MR.fan(K, N, hub), True))
    rnd = MR.random_mesh(K, N, 11 * N + 5)
    out += [("random", rnd, False), ("random+nodes", rnd, True)]
    return out


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, K, D, elem, node=None):
    key = (K, D, elem, node, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_mesh(C.byref(h), c.dtype, K, D, node.encode() if node else None, elem.encode(), log,
                                                  len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _upload(c, arrays):
    ptrs = (C.c_void_p * 4)()
    for slot, arr in arrays:
        dev = C.c_void_p()
        c.L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(dev)))
        ptrs[slot] = dev.value
    return ptrs


def _bind(c, K, D, el, with_node, rng):
    """compiles (once per process) and binds ASYM_ELEM (and NODE) with random per-element, per-node and per-unknown data;
    returns (id, x -> (g, all term values))"""
    L, n, dt = c.L, c.n, c.dt
    N, E = n // D, el.shape[0]
    p0 = (0.5 + rng.random(E)).astype(dt)
    p1 = (0.5 + rng.random(N)).astype(dt)
    p2 = rng.standard_normal(n).astype(dt)
    ptrs = _upload(c, ((0, p0), (1, p1), (2, p2)))
    cs = (C.c_double * 8)(*(MR.SCALARS + (0.0,) * 5))
    oid = C.c_int(-1)
    ke, pe = _i32(el)
    h = _compile(c, K, D, MR.ASYM_ELEM, MR.NODE if with_node else None)
    L.check(c.core.lbfgsx_objective_bind_mesh(c.h, h, E, pe, 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
    ke[:] = -5  # the binding keeps its own copy
    assert oid.value == L.OBJ_BOUND

    def ref(x):
        tg, v = MR.asym_elem_terms(x, el, D, p0, p1)
        if not with_node:
            return MR.mesh_grad(tg, el, N), v
        ng, nv = MR.node_terms(x, D, p2)
        return MR.mesh_grad(tg, el, N, ng), np.concatenate([v, nv])
    return oid.value, ref


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,K,D,N", _shapes())
def test_eval_and_trial_statements_in_both_tile_orders(A, dtype, K, D, N):
    rng = np.random.default_rng(100 + N)
    n = N * D
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        xp = rng.standard_normal(n).astype(dt)
        d = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, xp)
        c.up(L.VEC_D, d)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        stale = np.full(n, -77.0, dt)
        step = 0.37
        xt_ref = R.axpy_ref(xp, d, step)
        for name, el, with_node in _families(K, N):
            oid, ref = _bind(c, K, D, el, with_node, rng)
            fx, g2, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g_ref, terms = ref(xp)
            _bits(c.down(L.VEC_G), g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(g2.value, g_ref, g_ref, dt, name + ": g.g")
            _dot_ok(x2.value, xp, xp, dt, name + ": x.x")
            g_ref, terms = ref(xt_ref)
            runs = []
            for k in range(2):
                c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible; a gather of it would show
                c.up(L.VEC_GT, stale)
                fx, dg = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                assert _launches(c.core) == before + 1
                _bits(c.down(L.VEC_XT), xt_ref, "%s launch %d: x trial" % (name, k))
                _bits(c.down(L.VEC_GT), g_ref, "%s launch %d: g trial" % (name, k))
                runs.append((fx.value, dg.value))
            assert runs[0] == runs[1], name + ": f or g.d depends on the tile order"
            _sum_ok(runs[0][0], terms, dt, name + ": f trial")
            _dot_ok(runs[0][1], g_ref, d, dt, name + ": g.d")
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,K,D,N", _shapes())
def test_b_eval_and_dg_maxstep_trial_statements(A, monkeypatch, dtype, K, D, N):
    """lbfgsx_b_eval, then the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d
    that lbfgsx_trial then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    rng = np.random.default_rng(300 + N)
    n = N * D
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for name, el, with_node in _families(K, N):
            oid, ref = _bind(c, K, D, el, with_node, rng)
            for which, arr in ((L.VEC_X, x), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                c.up(which, arr)
            fx, pg, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g_ref, terms = ref(x)
            _bits(c.down(L.VEC_G), g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(x2.value, x, x, dt, name + ": x.x")
            assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), name
            c.up(L.VEC_G, g0)
            L.check(c.core.lbfgsx_ls_begin(c.h))
            runs0, hits0 = _ahead(c)
            dg, sm = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
            assert _launches(c.core) == before + 1
            assert _ahead(c) == (runs0 + 1, hits0), name + ": the fused kernel did not run"
            g_ref, terms = ref(xt_ref)
            _bits(c.down(L.VEC_XT), xt_ref, name + ": x trial left by the fused pass")
            _bits(c.down(L.VEC_GT), g_ref, name + ": g trial left by the fused pass")
            fx, dgt = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
            assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)
            _bits(c.down(L.VEC_G), g0, name + ": g at xp is left alone")
            _dot_ok(dg.value, g0, d, dt, name + ": g.d")
            assert sm.value == R.step_max_ref(x, d, lb, ub), name
            _sum_ok(fx.value, terms, dt, name + ": f trial")
            _dot_ok(dgt.value, g_ref, d, dt, name + ": grad(x).d")


# ---------------------------------------------------------------- cross-form identities
def _eval_and_two_trials(c, oid):
    L = c.L
    fx, g2, x2 = _d(3)
    L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
    got = [c.down(L.VEC_G).copy(), fx.value, g2.value, x2.value]
    L.check(c.core.lbfgsx_ls_begin(c.h))
    for k in range(2):
        ft, dg = _d(2)
        L.check(c.core.lbfgsx_trial(c.h, oid, 0.37, C.byref(ft), C.byref(dg)))
        got += [c.down(L.VEC_GT).copy(), c.down(L.VEC_XT).copy(), ft.value, dg.value]
    return got


def _same(a, b, what):
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            _bits(v, u, what)
        else:
            assert u == v, what


def _graph_families(n):
    return [("reversed-path", *GR.reversed_path(n)), ("star", *GR.star(n, n // 2)), ("random", *GR.random_multigraph(n, 11 * n + 5)),
            ("ring-chords", *GR.ring_chords(n))]


@pytest.mark.parametrize("dtype,n", [pytest.param(dt, n, id="%s-%d" % ("f64" if dt == O.F64 else "f32", n))
                                     for dt in (O.F64, O.F32) for n in (3, 64 * PACK[dt] + 1, 512 * PACK[dt] + 3,
                                                                        5 * 512 * PACK[dt] + PACK[dt] + 1)])
def test_a_two_node_scalar_mesh_is_the_graph_of_the_same_body(A, dtype, n):
    """K = 2, D = 1: ASYM_EDGE after the line that names v[0] and v[1] i and j is the element body, the edges are the
    elements.  g, x, f and the sums are bit-identical to the GraphObjective's, from lbfgsx_eval and both trial orders"""
    rng = np.random.default_rng(500 + n)
    dt = NPDT[dtype]
    x, d = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    with Ctx(A, dtype, n) as c:
        L = c.L
        c.up(L.VEC_X, x)
        c.up(L.VEC_D, d)
        for name, ei, ej in _graph_families(n):
            E = ei.size
            p0, p1 = (0.5 + rng.random(E)).astype(dt), (0.5 + rng.random(n)).astype(dt)
            ptrs = _upload(c, ((0, p0), (1, p1)))
            cs = (C.c_double * 8)(*(GR.SCALARS + (0.0,) * 5))
            hg = C.c_void_p()
            log = C.create_string_buffer(8192)
            for node in (None, GR.NODE):
                assert c.core.lbfgsx_objective_compile_graph(C.byref(hg), dtype, node.encode() if node else None,
                                                             GR.ASYM_EDGE.encode(), log, len(log)) == 0, log.value
                oid = C.c_int(-1)
                i32p = C.POINTER(C.c_int32)
                ki, kj = np.ascontiguousarray(ei, np.int32), np.ascontiguousarray(ej, np.int32)
                L.check(c.core.lbfgsx_objective_bind_graph(c.h, hg, E, ki.ctypes.data_as(i32p), kj.ctypes.data_as(i32p), 0,
                                                           C.byref(ptrs), C.byref(cs), C.byref(oid)))
                want = _eval_and_two_trials(c, oid.value)
                el = np.stack([ei, ej], 1)
                hm = _compile(c, 2, 1, MR.ALIAS_IJ + GR.ASYM_EDGE, node)
                L.check(c.core.lbfgsx_objective_bind_mesh(c.h, hm, E, _i32(el)[1], 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
                got = _eval_and_two_trials(c, oid.value)
                _same(want, got, "%s: mesh against graph" % name)
                assert np.any(got[0] != 0)
                c.core.lbfgsx_objective_destroy(hg)


@pytest.mark.parametrize("dtype,n", [pytest.param(dt, n, id="%s-%d" % ("f64" if dt == O.F64 else "f32", n))
                                     for dt in (O.F64, O.F32) for n in (3, 4, 64 * PACK[dt] + 1, 512 * PACK[dt] + 3,
                                                                        5 * 512 * PACK[dt] + PACK[dt] + 1)])
def test_the_scalar_strip_is_the_chain_of_the_same_body(A, dtype, n):
    """K = 3, D = 1, elements (t, t+1, t+2) with e = t: the K = 3 chain body TRIPLE after the line that names e i is the
    element body.  grad, x and f are bit-identical to the ChainObjective's, and the gradient is the restatement's"""
    rng = np.random.default_rng(600 + n)
    dt = NPDT[dtype]
    p0 = (0.5 + rng.random(n)).astype(dt)
    x, d = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    el = MR.strip(3, n)
    with Ctx(A, dtype, n) as c:
        L = c.L
        ptrs = _upload(c, ((0, p0),))
        c.up(L.VEC_X, x)
        c.up(L.VEC_D, d)
        hc = C.c_void_p()
        log = C.create_string_buffer(8192)
        assert c.core.lbfgsx_objective_compile_chain(C.byref(hc), dtype, 3, MR.TRIPLE.encode(), log, len(log)) == 0, log.value
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind(c.h, hc, C.byref(ptrs), None, C.byref(oid)))
        want = _eval_and_two_trials(c, oid.value)
        L.check(c.core.lbfgsx_objective_bind_mesh(c.h, _compile(c, 3, 1, MR.ALIAS_I + MR.TRIPLE), el.shape[0], _i32(el)[1], 0,
                                                  C.byref(ptrs), None, C.byref(oid)))
        got = _eval_and_two_trials(c, oid.value)
        c.core.lbfgsx_objective_destroy(hc)
    _same(want, got, "mesh against chain")
    _bits(got[0], MR.mesh_grad(MR.triple_terms(x, el, p0)[0], el, n), "g against the restatement")
    assert np.any(got[0] != 0)


# ---------------------------------------------------------------- the topology
def _read_topology(c, N, K, E):
    gotE = C.c_int64(-1)
    off, words = np.full(N + 1, 7, np.uint32), np.full((K * E, K), 7, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    c.L.check(c.core.lbfgsx_objective_mesh_topology(c.h, C.byref(gotE), off.ctypes.data_as(u32p), words.ctypes.data_as(u32p)))
    return gotE.value, off, words


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("size", ["K", "K+1", "129", "1031"])
def test_topology_is_the_incidence_list_of_the_restatement(A, K, size):
    N, D = {"K": K, "K+1": K + 1}.get(size) or int(size), 2
    with Ctx(A, O.F64, N * D) as c:
        L = c.L
        meshes = [("fan-%d" % hub, MR.fan(K, N, hub)) for hub in dict.fromkeys((0, N // 2, N - 1))]
        meshes += [("random", MR.random_mesh(K, N, 3 * N + 1)), ("reversed-strip", MR.reversed_strip(K, N))]
        for name, el in meshes:
            E = el.shape[0]
            oid = C.c_int(-1)
            ke, pe = _i32(el)
            L.check(c.core.lbfgsx_objective_bind_mesh(c.h, _compile(c, K, D, MR.PAIRS_ELEM), E, pe, 0, None, None, C.byref(oid)))
            ke[:] = -5  # the binding keeps its own copy
            gotE, off, words = _read_topology(c, N, K, E)
            roff, rwords = MR.incidence(el, N)
            assert gotE == E, name
            assert np.array_equal(off, roff) and np.array_equal(words, rwords), name


def test_elements_may_be_a_device_array(A):
    """elems_on_device = 1: the same list from a device copy of the table (here: one of the context's own data buffers, which
    holds the int32 indices as raw bytes)"""
    K, D, N = 3, 1, 640
    el = MR.random_mesh(K, N, 9)
    E = el.shape[0]
    with Ctx(A, O.F32, N * D) as c:  # f32: an element of a data buffer is 4 bytes, as an index
        L = c.L
        dev = C.c_void_p()
        raw = np.ascontiguousarray(el, np.int32)
        L.check(c.core.lbfgsx_objective_upload_count(c.h, 3, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(dev)))
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind_mesh(c.h, _compile(c, K, D, MR.PAIRS_ELEM), E, dev, 1, None, None, C.byref(oid)))
        _, off, words = _read_topology(c, N, K, E)
    roff, rwords = MR.incidence(el, N)
    assert np.array_equal(off, roff) and np.array_equal(words, rwords)


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "mesh_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _triangle_instance(A, rows, cols, k):
    """tests/cpp/mesh_probe.cpp: the mesh, the rest values, start() and the box, operation for operation"""
    tri, pos = MR.lattice(3, (rows, cols))
    N = rows * cols
    p = pos[tri]
    l = [((p[:, (j + 1) % 3] - p[:, j]) ** 2).sum(1) for j in range(3)]
    rest = pos.reshape(-1)
    f = A.MeshObjective(MR.TRIANGLE, tri, 2, node_body=MR.TIE_NODE, data=(l[0], l[1], l[2], rest), scalars=(k["c0"], k["c1"], k["c2"]))
    t = (np.arange(N, dtype=np.float64) + 1.0) / float(N + 1)
    bump = (12.0 * ((t * (1.0 - t)) * (0.5 - t))) * (1.0 + 0.5 * t)
    x0 = np.stack([pos[:, 0] + k["amp"] * bump, pos[:, 1] + (k["amp"] * 0.5) * (bump * (1.0 - t))], 1).reshape(-1)
    return f, x0, rest + k["lo"], rest + k["hi"]


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%d" % (i["solver"], i["n"]))
def test_triangle_energy_follows_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
    assert inst["iterations"] >= 8
    f, x0, lb, ub = _triangle_instance(A, inst["rows"], inst["cols"], _golden()["constants"])
    assert np.any(x0 < lb) and np.any(x0 > ub)  # bounds are active at the projected start
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = x0.copy()
        if inst["solver"] == "lbfgs":
            s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
            niter, fx = s.minimize(f, x)
        else:
            s = A.LBFGSBSolver(A.LBFGSBParam(past=0, **prm))
            niter, fx = s.minimize(f, x, lb, ub)
        x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
        assert x_ref.size == n
        dx, df = float(np.abs(x - x_ref).max()), abs(fx - inst["f"][k - 1])
        print("k %d: niter %d nfev %d |dx| %.3g |df| %.3g" % (k, niter, s.last.nfev, dx, df))
        assert (niter, s.last.nfev) == (inst["niter"][k - 1], inst["nfev"][k - 1])
        assert dx <= tol and df <= tol


def test_cpp_mesh_objective_follows_the_reference(tmp_path):
    """tests/cpp/mesh_probe.cpp with MeshObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "mesh_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DMESH_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "mesh_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["rows"], i["cols"]) for i in insts}):
        mine = [i for i in insts if (i["rows"], i["cols"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe, str(shape[0]), str(shape[1]), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=300)
        assert out.returncode == 0 and "MESH PROBE OK" in out.stdout, out.stdout[-2000:]
        rows_ = {}
        for line in out.stdout.splitlines():
            w = line.split()
            if w and w[0] in ("lbfgs", "lbfgsb"):
                rows_[(w[0], int(w[1]))] = (int(w[2]), float(w[4]), np.array([float(v) for v in w[5:]]))
        for inst in mine:
            for k in range(1, inst["iterations"] + 1):
                niter, fx, x = rows_[(inst["solver"], k)]
                x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
                assert niter == inst["niter"][k - 1]
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], shape, k)


# ---------------------------------------------------------------- convergence
@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_convex_instance_converges_to_the_linear_solve(A, solver):
    """f = sum over triangles of w/2 (|x_a - x_b|^2 over the three node pairs) + sum over nodes of 1/2 |x_v - b_v|^2, D = 2, on
    the random mesh: the minimiser solves (I + L_w) x = b per unknown, L_w the weighted Laplacian of the triangles' edges (a
    duplicate element counts twice).  The solver ends by its own gradient test, and the gradient recomputed in numpy from the
    dense matrix meets that test within a factor 2 (another summation order), as in the graph test of the same name.
    b = 1 + 0.01 N(0, 1): f is small at the minimiser, so that decreases of order (eps ||x||)^2 stay visible in its values"""
    K, D, N, eps, cap = 3, 2, 200, 1e-8, 2000
    n = N * D
    el = MR.random_mesh(K, N, 2024)
    rng = np.random.default_rng(5)
    w, b = 0.5 + rng.random(el.shape[0]), 1.0 + 0.01 * rng.standard_normal(n)
    M = np.eye(N)
    for e in range(el.shape[0]):
        for a in range(K):
            for bb in range(a + 1, K):
                i, j = el[e, a], el[e, bb]
                M[i, i] += w[e]
                M[j, j] += w[e]
                M[i, j] -= w[e]
                M[j, i] -= w[e]
    M = np.kron(M, np.eye(D))  # node-major unknowns
    x_star = np.linalg.solve(M, b)
    f = A.MeshObjective(MR.PAIRS_ELEM, el, D, node_body=MR.FIDELITY_NODE, data=(w, b))
    x = np.zeros(n)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
        measure = float(np.linalg.norm(M @ x - b))
    else:
        lb, ub = np.full(n, -50.0), np.full(n, 50.0)
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        niter, fx = s.minimize(f, x, lb, ub)
        g = M @ x - b
        measure = float(np.abs(np.clip(x - g, lb, ub) - x).max())
        assert np.abs(x).max() < 50.0
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    err = float(np.abs(x - x_star).max())
    print("%s: niter %d nfev %d fx %.12g stopping measure %.3g (bound %.3g) ||g||_2 %.3g |x - x*| %.3g"
          % (solver, niter, s.last.nfev, fx, measure, bound, float(np.linalg.norm(M @ x - b)), err))
    assert 0 < niter < cap
    assert measure <= 2.0 * bound
    assert err <= 1e-6


# ---------------------------------------------------------------- launch accounting
def _strip_pair(A, n):
    """PAIR as the path graph and, after the line that names v[0] and v[1] i and j, as the K = 2, D = 1 strip: equal values
    and gradients (test_a_two_node_scalar_mesh_is_the_graph_of_the_same_body), so both solves take the same path"""
    rng = np.random.default_rng(n)
    p0 = 0.5 + rng.random(n)
    x0 = 0.5 * rng.standard_normal(n)
    return x0, (("graph", A.GraphObjective(GR.PAIR, edges=GR.path(n), data=(p0,))),
                ("mesh", A.MeshObjective(MR.ALIAS_IJ + GR.PAIR, MR.strip(2, n), 1, data=(p0,))))


def test_mesh_solve_issues_the_launches_per_iteration_of_a_graph_solve(A):
    """the same iterates and the same launches, the bind's included (both builds are a validation, an expansion, a sort, the
    offsets and the entries)"""
    core, _ = A.load()
    n, m = 200_001, 6
    x0, objs = _strip_pair(A, n)
    out = {}
    for name, f in objs:
        for iters in (10, 20):
            s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0, epsilon_rel=0, max_iterations=iters), linesearch=A.LS_MORE_THUENTE)
            s.prepare(n)
            x = x0.copy()
            c0 = _counters(core)
            niter, fx = s.minimize(f, x)
            c1 = _counters(core)
            out[name, iters] = (niter, s.last.nfev, fx, c1[0] - c0[0], c1[3] - c0[3])
    print(out)
    for iters in (10, 20):
        assert out["mesh", iters][:3] == out["graph", iters][:3] and out["mesh", iters][0] == iters
        # the byte model (launch_args.hpp): a trial launch reads xp and d, writes x and grad and reads the one data array; a
        # mesh's adds the N + 1 offsets, the K E entries of 4 K bytes and (K - 1) D gathered values of xp and of d per entry
        # -- at K = 2, D = 1 what the graph's adds.  Every evaluation but the first is a trial launch
        trials, E, K, D = out["mesh", iters][1] - 1, n - 1, 2, 1
        assert out["mesh", iters][4] == trials * (n * 8 * 5 + (n // D + 1) * 4 + K * E * 4 * K + K * E * (K - 1) * D * 8 * 2)
        assert out["mesh", iters][4] == out["graph", iters][4]
    assert out["mesh", 20][3] - out["mesh", 10][3] == out["graph", 20][3] - out["graph", 10][3] > 0
    assert out["mesh", 10][3] == out["graph", 10][3]  # the bind's launches too


def test_lbfgsb_mesh_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    n, m, iters = 20_001, 6, 25
    x0, objs = _strip_pair(A, n)
    lb, ub = np.full(n, -0.5), np.full(n, 0.9)
    x0 = np.clip(x0, lb, ub)
    out = {}
    for name, f in objs:
        s = A.LBFGSBSolver(A.LBFGSBParam(m=m, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
        s.prepare(n)
        x = x0.copy()
        niter, fx = s.minimize(f, x, lb, ub)
        ahead = (C.c_int64 * 2)()
        assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
        out[name] = (niter, s.last.nfev, fx, ahead[0], ahead[1])
    print(out)
    assert out["mesh"][3] > 0 and out["mesh"][4] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["mesh"][3] == out["mesh"][0]           # on every iteration's first trial
    assert out["mesh"] == out["graph"]


# ---------------------------------------------------------------- refusals
def _nothing_bound(c):
    fx, g2, x2 = _d(3)
    before = _launches(c.core)
    assert c.core.lbfgsx_eval(c.h, c.L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
    assert _launches(c.core) == before
    assert c.core.lbfgsx_objective_mesh_topology(c.h, None, None, None) == c.L.E_INVALID


def test_offending_elements_are_refused_by_value_and_nothing_is_evaluated(A):
    K, D, N = 3, 2, 10
    good = [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 6]]
    with Ctx(A, O.F64, N * D) as c:
        L = c.L
        h = _compile(c, K, D, MR.PAIRS_ELEM)

        def bind(el, E=None, handle=h, oid=None):
            return c.core.lbfgsx_objective_bind_mesh(c.h, handle, len(el) if E is None else E, _i32(el)[1], 0, None, None, oid)
        cases = [("repeated node", 3, [7, 2, 7], "element e = 3 is (7, 2, 7) with N = 10"),
                 ("index -1", 1, [-1, 4, 5], "element e = 1 is (-1, 4, 5) with N = 10"),
                 ("index N", 4, [2, 10, 3], "element e = 4 is (2, 10, 3) with N = 10")]
        for name, e, row, what in cases:
            assert bind(good) == 0  # something is bound before each refusal
            el = [list(r) for r in good]
            el[e] = row
            before = _launches(c.core)
            rc = bind(el, oid=C.byref(C.c_int(-1)))
            assert rc == L.E_INVALID and what in L.last_error() and "1 of the E = 5 elements" in L.last_error(), L.last_error()
            assert _launches(c.core) == before + 1, name + ": only the validation kernel runs on unchecked indices"
            _nothing_bound(c)
        # two offenders: the count, and the smaller e
        rc = bind([[0, 1, 2], [1, 2, 3], [12, 3, 4], [3, 3, 5], [4, 5, 6]])
        assert rc == L.E_INVALID and "element e = 2 is (12, 3, 4)" in L.last_error() and "2 of the E = 5" in L.last_error()
        for E, what in ((0, "E = 0"), (-3, "E = -3"), (2 ** 30, "E = 1073741824 exceeds 2^30 - 1")):
            assert bind(good) == 0
            assert bind(good, E=E) == L.E_INVALID and what in L.last_error(), L.last_error()
            _nothing_bound(c)
        assert bind(good) == 0
        fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
        assert bind(good, handle=fc.compile()) == L.E_INVALID
        assert "the handle is a chain objective, not a mesh objective" in L.last_error()
        _nothing_bound(c)
        assert bind(good) == 0
        f32 = A.MeshObjective(MR.PAIRS_ELEM, good, D)
        assert bind(good, handle=f32.compile(np.float32)) == L.E_INVALID and "the other dtype" in L.last_error()
        _nothing_bound(c)
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID
        assert "a mesh objective is bound with its elements: lbfgsx_objective_bind_mesh" in L.last_error()
        i32p = C.POINTER(C.c_int32)
        e0 = np.zeros(5, np.int32).ctypes.data_as(i32p)
        assert c.core.lbfgsx_objective_bind_graph(c.h, h, 5, e0, e0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a mesh objective, not a graph objective" in L.last_error()
        # and a good table binds
        oid = C.c_int(-1)
        assert bind(good, oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
    with Ctx(A, O.F64, 2 * 10 + 1) as c:  # n is not a multiple of D
        rc = c.core.lbfgsx_objective_bind_mesh(c.h, _compile(c, K, D, MR.PAIRS_ELEM), 5, _i32(good)[1], 0, None, None, None)
        assert rc == c.L.E_INVALID and "n = 21 is not a multiple of D = 2" in c.L.last_error()
        _nothing_bound(c)
    # through the solver: ValueError with the element named
    for el, what in (([[0, 1, 2], [4, 3, 4]], "element e = 1 is \\(4, 3, 4\\) with N = 6"),
                     ([[0, 1, 2], [-1, 2, 3]], "element e = 1 is \\(-1, 2, 3\\) with N = 6"),
                     ([[0, 6, 1], [1, 2, 3]], "element e = 0 is \\(0, 6, 1\\) with N = 6")):
        with pytest.raises(ValueError, match=what):
            A.LBFGSSolver(A.LBFGSParam()).minimize(A.MeshObjective(MR.PAIRS_ELEM, el, 2, data=(np.ones(2),)), np.zeros(12))


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    tri, pos = MR.lattice(3, (10, 10))
    f = A.MeshObjective(MR.PAIRS_ELEM, tri, 2, node_body=MR.FIDELITY_NODE, data=(np.ones(tri.shape[0]), pos.reshape(-1)))
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, np.zeros(200))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, np.zeros(200))
