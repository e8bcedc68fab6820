"""-m gpu: graph objectives (lbfgspp_amd.GraphObjective, csrc/graph_kernels.cuh, csrc/graph_topology.hip) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders), lbfgsx_b_eval and
    lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/graph_ref.py -- gradient and written x bit for bit, f and
    the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal -- on paths, reversed paths,
    stars, random multigraphs and the ring with chords, all bound one after another to one context (the list is rebuilt at
    every bind);
  * the path graph with a K = 2 chain body as its edge body is that ChainObjective bit for bit;
  * lbfgsx_objective_topology is the incidence list of the restatement;
  * the double-well energy on the ring with chords follows the reference (tests/golden/graph_golden.json), from Python and C++;
  * a convex instance converges to the solution of its linear system under both solvers; launch accounting; refusals."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import graph_ref as GR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_term_objective_gpu import _counters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates of a 16-byte pack
TRIAL_U = 2                  # graph_kernels.cuh: kGraphTrialU, the tile depth of the two trial kernels


def _size_list(dtype):
    W = PACK[dtype]
    tile = 256 * TRIAL_U  # packs
    # around a wave, a block and one and two trial tiles, with and without tail coordinates; about five tiles: several blocks,
    # and both tile orders cross tile borders.  2 and 3 have no whole pack at f32 (at f64 W = 2 and an edge needs two nodes:
    # there is no smaller graph); 3 and 64 W + 1 have exactly one coordinate past the last pack; tile W + 1 is one node past
    # one trial tile
    return [2, 3, 64 * W - 1, 64 * W + 1, 256 * W + W + 1, tile * W + 1, tile * W + 3, 2 * tile * W + W + 1, 5 * tile * W + W + 1]


def _sizes():
    return [pytest.param(dtype, n, id="%s-%d" % ("f64" if dtype == O.F64 else "f32", n))
            for dtype in (O.F64, O.F32) for n in _size_list(dtype)]


def _families(n):
    """(name, ei, ej, with the node body)"""
    out = [("reversed-path", *GR.reversed_path(n), False)]
    for hub in dict.fromkeys((0, n // 2, n - 1)):  # n - 1 is a tail coordinate when n is no multiple of W
        out.append(("star-%d" % hub, *GR.star(n, hub), True))
    rnd = GR.random_multigraph(n, 11 * n + 5)
    out += [("random", *rnd, False), ("random+nodes", *rnd, True), ("ring-chords", *GR.ring_chords(n), True)]
    return out


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, edge, node=None):
    key = (edge, node, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_graph(C.byref(h), c.dtype, node.encode() if node else None, edge.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _bind(c, ei, ej, with_node, rng):
    """compiles (once per process) and binds ASYM_EDGE (and NODE) with random per-edge and per-node weights; returns
    (id, x -> (g, all term values))"""
    L, n, dt = c.L, c.n, c.dt
    E = ei.size
    p0 = (0.5 + rng.random(E)).astype(dt)
    p1 = (0.5 + rng.random(n)).astype(dt)
    ptrs = (C.c_void_p * 4)()
    for slot, arr in ((0, p0), (1, p1)):
        dev = C.c_void_p()
        L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(dev)))
        ptrs[slot] = dev.value
    cs = (C.c_double * 8)(*(GR.SCALARS + (0.0,) * 5))
    oid = C.c_int(-1)
    (ki, pi), (kj, pj) = _i32(ei), _i32(ej)
    h = _compile(c, GR.ASYM_EDGE, GR.NODE if with_node else None)
    L.check(c.core.lbfgsx_objective_bind_graph(c.h, h, E, pi, pj, 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
    ki[:] = -5  # the binding keeps its own copy
    kj[:] = -5
    assert oid.value == L.OBJ_BOUND

    def ref(x):
        tg, v = GR.asym_edge_terms(x, ei, ej, p0, p1)
        if not with_node:
            return GR.graph_grad(tg, ei, ej, n), v
        ng, nv = GR.node_terms(x, p1)
        return GR.graph_grad(tg, ei, ej, n, ng), np.concatenate([v, nv])
    return oid.value, ref


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,n", _sizes())
def test_eval_statement(A, dtype, n):
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        x = rng.standard_normal(n).astype(dt)
        c.up(L.VEC_X, x)
        for name, ei, ej, with_node in _families(n):
            oid, ref = _bind(c, ei, ej, with_node, rng)
            fx, g2, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g = c.down(L.VEC_G)
            g_ref, terms = ref(x)
            _bits(g, g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(g2.value, g_ref, g_ref, dt, name + ": g.g")
            _dot_ok(x2.value, x, x, dt, name + ": x.x")


@pytest.mark.parametrize("dtype,n", _sizes())
def test_trial_statement_in_both_tile_orders(A, dtype, n):
    rng = np.random.default_rng(200 + n)
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
        for name, ei, ej, with_node in _families(n):
            oid, ref = _bind(c, ei, ej, with_node, rng)
            g_ref, terms = ref(xt_ref)
            runs = []
            for k in range(2):
                c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible; a gather of it would show
                c.up(L.VEC_GT, stale)
                fx, dg = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                assert _launches(c.core) == before + 1
                xt, gt = c.down(L.VEC_XT), c.down(L.VEC_GT)
                _bits(xt, xt_ref, "%s launch %d: x trial" % (name, k))
                _bits(gt, g_ref, "%s launch %d: g trial" % (name, k))
                runs.append((fx.value, dg.value))
            assert runs[0] == runs[1], name + ": f or g.d depends on the tile order"
            _sum_ok(runs[0][0], terms, dt, name + ": f")
            _dot_ok(runs[0][1], g_ref, d, dt, name + ": g.d")
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,n", _sizes())
def test_b_eval_statement(A, dtype, n):
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        x, _, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        c.up(L.VEC_X, x)
        c.up(L.VEC_LB, lb)
        c.up(L.VEC_UB, ub)
        for name, ei, ej, with_node in _families(n):
            oid, ref = _bind(c, ei, ej, with_node, rng)
            fx, pg, x2 = _d(3)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
            assert _launches(c.core) == before + 1
            g = c.down(L.VEC_G)
            g_ref, terms = ref(x)
            _bits(g, g_ref, name + ": g")
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(x2.value, x, x, dt, name + ": x.x")
            assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), name


@pytest.mark.parametrize("dtype,n", _sizes())
def test_dg_maxstep_trial_statement(A, monkeypatch, dtype, n):
    """the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d that lbfgsx_trial
    then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    rng = np.random.default_rng(400 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for name, ei, ej, with_node in _families(n):
            oid, ref = _bind(c, ei, ej, with_node, rng)
            for which, arr in ((L.VEC_X, x), (L.VEC_G, g0), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                c.up(which, arr)
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
            _sum_ok(fx.value, terms, dt, name + ": f")
            _dot_ok(dgt.value, g_ref, d, dt, name + ": grad(x).d")


# ---------------------------------------------------------------- the path graph is a chain
@pytest.mark.parametrize("dtype,n", _sizes())
def test_path_graph_is_the_chain_of_the_same_body(A, dtype, n):
    """edges (t, t+1) with e = t: the K = 2 chain body PAIR, unchanged, is the edge body (its i is the term's start in both
    forms).  grad and f are bit-identical to the ChainObjective's, from lbfgsx_eval and from lbfgsx_trial in both tile orders,
    and the gradient is the restatement's"""
    rng = np.random.default_rng(500 + n)
    dt = NPDT[dtype]
    p0 = (0.5 + rng.random(n)).astype(dt)
    x = rng.standard_normal(n).astype(dt)
    d = rng.standard_normal(n).astype(dt)
    ei, ej = GR.path(n)
    got = {}
    with Ctx(A, dtype, n) as c:
        L = c.L
        ptrs = (C.c_void_p * 4)()
        dev = C.c_void_p()
        L.check(c.core.lbfgsx_objective_upload(c.h, 0, p0.ctypes.data_as(C.c_void_p), C.byref(dev)))
        ptrs[0] = dev.value
        c.up(L.VEC_X, x)
        c.up(L.VEC_D, d)
        hc = C.c_void_p()
        log = C.create_string_buffer(8192)
        assert c.core.lbfgsx_objective_compile_chain(C.byref(hc), dtype, 2, GR.PAIR.encode(), log, len(log)) == 0, log.value
        oid = C.c_int(-1)
        for name in ("chain", "graph"):
            if name == "chain":
                L.check(c.core.lbfgsx_objective_bind(c.h, hc, C.byref(ptrs), None, C.byref(oid)))
            else:
                L.check(c.core.lbfgsx_objective_bind_graph(c.h, _compile(c, GR.PAIR), ei.size, _i32(ei)[1], _i32(ej)[1], 0,
                                                           C.byref(ptrs), None, C.byref(oid)))
            fx, g2, x2 = _d(3)
            L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
            got[name] = [c.down(L.VEC_G).copy(), fx.value, g2.value]
            L.check(c.core.lbfgsx_ls_begin(c.h))
            for k in range(2):
                ft, dg = _d(2)
                L.check(c.core.lbfgsx_trial(c.h, oid.value, 0.37, C.byref(ft), C.byref(dg)))
                got[name] += [c.down(L.VEC_GT).copy(), c.down(L.VEC_XT).copy(), ft.value, dg.value]
        c.core.lbfgsx_objective_destroy(hc)
    for a, b in zip(got["chain"], got["graph"]):
        if isinstance(a, np.ndarray):
            _bits(b, a, "graph against chain")
        else:
            assert a == b
    _bits(got["graph"][0], GR.graph_grad(GR.pair_terms(x, ei, ej, p0)[0], ei, ej, n), "g against the restatement")
    assert np.any(got["graph"][0] != 0)


# ---------------------------------------------------------------- the topology
@pytest.mark.parametrize("n", [2, 3, 129, 1031])
def test_topology_is_the_incidence_list_of_the_restatement(A, n):
    with Ctx(A, O.F64, n) as c:
        L = c.L
        graphs = [("star-%d" % hub, *GR.star(n, hub)) for hub in dict.fromkeys((0, n // 2, n - 1))]
        graphs += [("random", *GR.random_multigraph(n, 3 * n + 1)), ("ring-chords", *GR.ring_chords(n))]
        for name, ei, ej in graphs:
            E = ei.size
            oid = C.c_int(-1)
            L.check(c.core.lbfgsx_objective_bind_graph(c.h, _compile(c, GR.SPRING_EDGE), E, _i32(ei)[1], _i32(ej)[1], 0, None, None,
                                                       C.byref(oid)))
            gotE = C.c_int64(-1)
            off, other, es = np.full(n + 1, 7, np.uint32), np.full(2 * E, 7, np.int32), np.full(2 * E, 7, np.uint32)
            L.check(c.core.lbfgsx_objective_topology(c.h, C.byref(gotE), off.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     other.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     es.ctypes.data_as(C.POINTER(C.c_uint32))))
            roff, rother, res = GR.incidence(ei, ej, n)
            assert gotE.value == E, name
            assert np.array_equal(off, roff) and np.array_equal(other, rother) and np.array_equal(es, res), name


def test_edges_may_be_device_arrays(A):
    """edges_on_device = 1: the same list from device copies of ei and ej (here: two of the context's own data buffers, which
    hold the int32 indices as raw bytes)"""
    n = 640
    ei, ej = GR.random_multigraph(n, 9)
    E = ei.size
    with Ctx(A, O.F32, n) as c:  # f32: an element of a data buffer is 4 bytes, as an index
        L = c.L
        devs = []
        for slot, a in ((2, ei), (3, ej)):
            dev = C.c_void_p()
            raw = np.ascontiguousarray(a, np.int32)
            L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, raw.ctypes.data_as(C.c_void_p), E, C.byref(dev)))
            devs.append(C.cast(dev, C.POINTER(C.c_int32)))
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind_graph(c.h, _compile(c, GR.SPRING_EDGE), E, devs[0], devs[1], 1, None, None, C.byref(oid)))
        off, other, es = np.zeros(n + 1, np.uint32), np.zeros(2 * E, np.int32), np.zeros(2 * E, np.uint32)
        L.check(c.core.lbfgsx_objective_topology(c.h, None, off.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 other.ctypes.data_as(C.POINTER(C.c_int32)), es.ctypes.data_as(C.POINTER(C.c_uint32))))
    roff, rother, res = GR.incidence(ei, ej, n)
    assert np.array_equal(off, roff) and np.array_equal(other, rother) and np.array_equal(es, res)


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "graph_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _start(n):
    """tests/cpp/graph_probe.cpp: start(), operation for operation"""
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    return -0.1 + (12.0 * ((t * (1.0 - t)) * (0.5 - t))) * (1.0 + 0.5 * t)


def _double_well(A, n, c0):
    ei, ej = GR.ring_chords(n)
    return A.GraphObjective(GR.SPRING_EDGE, edges=(ei, ej), node_body=GR.WELL_NODE, data=(GR.ring_weights(ei.size),), scalars=(c0,))


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%d" % (i["solver"], i["n"]))
def test_double_well_follows_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
    c0 = _golden()["c0"]
    assert inst["iterations"] >= 8
    f = _double_well(A, n, c0)
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = _start(n)
        if inst["solver"] == "lbfgs":
            s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
            niter, fx = s.minimize(f, x)
        else:
            s = A.LBFGSBSolver(A.LBFGSBParam(past=0, **prm))
            niter, fx = s.minimize(f, x, np.full(n, inst["lb"]), np.full(n, inst["ub"]))
        x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
        dx, df = float(np.abs(x - x_ref).max()), abs(fx - inst["f"][k - 1])
        print("k %d: niter %d nfev %d |dx| %.3g |df| %.3g" % (k, niter, s.last.nfev, dx, df))
        assert (niter, s.last.nfev) == (inst["niter"][k - 1], inst["nfev"][k - 1])
        assert dx <= tol and df <= tol


def test_cpp_graph_objective_follows_the_reference(tmp_path):
    """tests/cpp/graph_probe.cpp with GraphObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "graph_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DGRAPH_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "graph_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for n in sorted({i["n"] for i in insts}):
        mine = [i for i in insts if i["n"] == n]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe, str(n), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "GRAPH PROBE OK" in out.stdout, out.stdout[-2000:]
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
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], n, k)


# ---------------------------------------------------------------- convergence
@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_convex_instance_converges_to_the_linear_solve(A, solver):
    """f = sum over edges of 1/2 w (x_i - x_j)^2 + sum over nodes of 1/2 (x - b)^2 on the random multigraph: the minimiser
    solves (I + L_w) x = b with L_w the weighted Laplacian (a duplicate edge counts twice).  The solver ends by its own
    gradient test, and the gradient recomputed in numpy from the dense matrix meets that test within a factor 2 (another
    summation order): ||g||_2 <= eps max(1, ||x||) for L-BFGS; for L-BFGS-B, whose own measure it is, ||P(x - g) - x||_inf,
    which with bounds that are never active is ||g||_inf.
    b = 1 + 0.01 N(0, 1): the line searches compare values of f, and a decrease of order (eps ||x||)^2 = 3e-14 is visible
    only where f itself is small.  At the minimiser f is about 1e-2 here (the springs are nearly relaxed); with b = N(0, 1) it
    is about 94, one ulp of which is 1.4e-14, and L-BFGS stalls at ||g|| = 4e-7 whatever evaluates the objective"""
    n, eps, cap = 300, 1e-8, 2000
    ei, ej = GR.random_multigraph(n, 2024)
    rng = np.random.default_rng(5)
    w, b = 0.5 + rng.random(ei.size), 1.0 + 0.01 * rng.standard_normal(n)
    M = np.eye(n)
    for e in range(ei.size):
        i, j = ei[e], ej[e]
        M[i, i] += w[e]
        M[j, j] += w[e]
        M[i, j] -= w[e]
        M[j, i] -= w[e]
    x_star = np.linalg.solve(M, b)
    f = A.GraphObjective(GR.SPRING_EDGE, edges=(ei, ej), node_body=GR.FIDELITY_NODE, data=(w, b))
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
def _path_pair(A, n):
    """PAIR as a chain and as the path graph (test_path_graph_is_the_chain_of_the_same_body: equal values and gradients, so
    both solves take the same path); a chain costs the launches of a built-in (test_chain_objective_gpu)"""
    rng = np.random.default_rng(n)
    p0 = 0.5 + rng.random(n)
    x0 = 0.5 * rng.standard_normal(n)
    return x0, (("chain", A.ChainObjective(GR.PAIR, K=2, data=(p0,))), ("graph", A.GraphObjective(GR.PAIR, edges=GR.path(n), data=(p0,))))


def test_graph_solve_issues_the_launches_per_iteration_of_a_chain_solve(A):
    """the same iterates, and the same launches for iterations 11 .. 20: what a graph solve adds is the build of its list at
    bind, once per solve whatever its length"""
    core, _ = A.load()
    n, m = 200_001, 6
    x0, objs = _path_pair(A, n)
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
        assert out["graph", iters][:3] == out["chain", iters][:3] and out["graph", iters][0] == iters
        # the byte model (launch_args.hpp): a trial launch reads xp and d, writes x and grad and reads the one data array; a
        # graph's adds the n + 1 offsets, the 2E entries of 8 bytes and 2E gathered values of xp and of d.  Every evaluation
        # but the first is a trial launch
        trials, E = out["graph", iters][1] - 1, n - 1
        assert out["chain", iters][4] == trials * (n * 8 * 5)
        assert out["graph", iters][4] == trials * (n * 8 * 5 + (n + 1) * 4 + 2 * E * 8 + 2 * E * 8 * 2)
    build = out["graph", 10][3] - out["chain", 10][3]
    assert 0 < build <= 8 and out["graph", 20][3] - out["chain", 20][3] == build
    assert out["graph", 20][3] - out["graph", 10][3] == out["chain", 20][3] - out["chain", 10][3] > 0


def test_lbfgsb_graph_takes_the_fused_dg_maxstep_trial(A):
    core, _ = A.load()
    n, m, iters = 20_001, 6, 25
    x0, objs = _path_pair(A, n)
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
    assert out["graph"][3] > 0 and out["graph"][4] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert out["graph"][3] == out["graph"][0]           # on every iteration's first trial
    assert out["graph"] == out["chain"]


# ---------------------------------------------------------------- refusals
def test_offending_edges_are_refused_by_value_and_nothing_is_evaluated(A):
    n = 10
    with Ctx(A, O.F64, n) as c:
        L = c.L
        h = _compile(c, GR.SPRING_EDGE)
        good_i, good_j = [0, 1, 2, 3, 4], [1, 2, 3, 4, 5]
        cases = [("self-loop", 3, 7, 7, "edge e = 3 is (i = 7, j = 7) with n = 10"),
                 ("index -1", 1, -1, 4, "edge e = 1 is (i = -1, j = 4) with n = 10"),
                 ("index n", 4, 2, 10, "edge e = 4 is (i = 2, j = 10) with n = 10")]
        for name, e, i, j, what in cases:
            ei, ej = list(good_i), list(good_j)
            ei[e], ej[e] = i, j
            oid = C.c_int(-1)
            before = _launches(c.core)
            rc = c.core.lbfgsx_objective_bind_graph(c.h, h, 5, _i32(ei)[1], _i32(ej)[1], 0, None, None, C.byref(oid))
            assert rc == L.E_INVALID and what in L.last_error() and "1 of the E = 5 edges" in L.last_error(), L.last_error()
            assert _launches(c.core) == before + 1, name + ": only the validation kernel runs on unchecked indices"
            # nothing is bound: the evaluation entry points have no objective to run
            fx, g2, x2 = _d(3)
            before = _launches(c.core)
            assert c.core.lbfgsx_eval(c.h, L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
            assert _launches(c.core) == before
            assert c.core.lbfgsx_objective_topology(c.h, None, None, None, None) == L.E_INVALID
        # two offenders: the count, and the smaller e
        rc = c.core.lbfgsx_objective_bind_graph(c.h, h, 5, _i32([0, 1, 12, 3, 4])[1], _i32([1, 2, 3, 3, 5])[1], 0, None, None, None)
        assert rc == L.E_INVALID and "edge e = 2 is (i = 12, j = 3)" in L.last_error() and "2 of the E = 5" in L.last_error()
        rc = c.core.lbfgsx_objective_bind_graph(c.h, h, 0, _i32(good_i)[1], _i32(good_j)[1], 0, None, None, None)
        assert rc == L.E_INVALID and "E = 0" in L.last_error()
        rc = c.core.lbfgsx_objective_bind_graph(c.h, h, 2 ** 31, _i32(good_i)[1], _i32(good_j)[1], 0, None, None, None)
        assert rc == L.E_INVALID and "E = 2147483648 exceeds 2^31 - 1" in L.last_error()
        fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
        rc = c.core.lbfgsx_objective_bind_graph(c.h, fc.compile(), 5, _i32(good_i)[1], _i32(good_j)[1], 0, None, None, None)
        assert rc == L.E_INVALID and "the handle is a chain objective, not a graph objective" in L.last_error()
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID
        assert "a graph objective is bound with its edges: lbfgsx_objective_bind_graph" in L.last_error()
        # and a good list binds
        oid = C.c_int(-1)
        assert c.core.lbfgsx_objective_bind_graph(c.h, h, 5, _i32(good_i)[1], _i32(good_j)[1], 0, None, None, C.byref(oid)) == 0
        assert oid.value == L.OBJ_BOUND
    # through the solver: ValueError with the edge named
    for ei, ej, what in (([0, 4], [1, 4], "edge e = 1 is \\(i = 4, j = 4\\) with n = 6"),
                         ([0, -1], [1, 2], "edge e = 1 is \\(i = -1, j = 2\\) with n = 6"),
                         ([0, 1], [6, 2], "edge e = 0 is \\(i = 0, j = 6\\) with n = 6")):
        with pytest.raises(ValueError, match=what):
            A.LBFGSSolver(A.LBFGSParam()).minimize(A.GraphObjective(GR.SPRING_EDGE, edges=(ei, ej), data=(np.ones(2),)), np.zeros(6))


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    f = _double_well(A, 1000, 1.0)
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, _start(1000))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, _start(1000))
    batch = B.LockstepBatch(A.LBFGSParam(m=3, max_iterations=3), 64, 2, dtype=np.float64)
    try:
        with pytest.raises(TypeError, match="fn must be callable"):
            batch.minimize_fn(_double_well(A, 64, 1.0), np.zeros((2, 64)))
    finally:
        batch.close()
