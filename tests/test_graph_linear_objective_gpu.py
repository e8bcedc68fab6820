"""-m gpu: graph-regularised linear-model objectives (lbfgspp_amd.GraphLinearObjective, csrc/linear_graph_kernels.cuh) on the
device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders, a stale trial vector in
    place), lbfgsx_b_eval and lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/graph_linear_ref.py -- gradient
    and written x bit for bit, f and the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly
    equal -- on n = 2 with one row and one edge, the 3 x 5 matrix with a multi-edge and an isolated node, random rows over a
    random multigraph with several lane counts, one coordinate past a trial tile, and long columns under a star whose hub is
    the dense column; two row bodies, an asymmetric and a symmetric edge body, each with and without the coordinate body.  The
    launches are counted: 11 per bind, 2 per evaluation, 3 with a long column, none for a trial handed out ahead;
  * both topology read-backs are the restatement's lists; a matrix and edges given as device arrays give the same bits;
  * linear-graph -> linear -> graph -> linear-graph on one context, each bit-equal to its own restatement;
  * offending edges and matrices are refused by value with nothing bound; refused modes say so;
  * both probe instances follow the reference (tests/golden/graph_linear_golden.json), from Python and C++;
  * Laplacian-regularised least squares converges to the solution of its normal equations; an L-BFGS-B solve with active bounds
    takes the fused dg / max-step / trial pass."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import graph_linear_ref as GL
import graph_ref as GR
import linear_ref as LR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates a thread owns (the values of a 16-byte pack)
GRAPH_LAUNCHES, LINEAR_LAUNCHES = 5, 6  # validation, expansion, sort, offsets, entries; those and the long-column search
BIND_LAUNCHES = GRAPH_LAUNCHES + LINEAR_LAUNCHES
# (row body, edge body, coordinate body): each body with and without the coordinate body
BODIES = [("cubic", "asym", False), ("cubic", "asym", True), ("hinge", "spring", False), ("hinge", "spring", True)]
LANES = {"pair": (0, 2), "tiny": (0, 4), "random": (0, 1, 8, 64), "tile": (0,), "long": (0,)}
CASES = [pytest.param(dt, name, id="%s-%s" % ("f64" if dt == O.F64 else "f32", name))
         for dt in (O.F64, O.F32) for name in ("pair", "tiny", "random", "tile", "long")]


def _problem(name, dtype):
    dt = NPDT[dtype]
    if name == "tile":
        return GL.tile(dt, PACK[dtype])
    return {"pair": GL.pair, "tiny": GL.tiny, "random": GL.random, "long": GL.long_columns}[name](dt)


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, row, edge, coord=None):
    key = (row, edge, coord, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_linear_graph(C.byref(h), c.dtype, coord.encode() if coord else None, edge.encode(),
                                                          row.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _info(c):
    info = (C.c_int64 * 8)()
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, C.byref(info), None, None, None, None, None, None))
    return dict(zip(("R", "nnz", "L", "C", "nlong", "nchunks"), list(info)[:6]))


def _upload(c, Q):
    """p0 per row, p2 per edge, p3 per node; returns the pointer and scalar arrays of a bind"""
    ptrs = (C.c_void_p * 4)()
    for slot, arr in ((0, Q.P.p0), (2, Q.p2), (3, Q.p3)):
        dev = C.c_void_p()
        c.L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, _vp(arr), arr.size, C.byref(dev)))
        ptrs[slot] = dev.value
    return ptrs, (C.c_double * 8)(*(Q.scalars + (0.0,) * (8 - len(Q.scalars))))


def _bind(c, Q, row, edge, with_ridge, lanes):
    """compiles (once per process) and binds the three bodies with Q's data; returns (id, L, x -> (g, terms))"""
    L, P = c.L, Q.P
    ptrs, cs = _upload(c, Q)
    oid = C.c_int(-1)
    rp, col, val, ei, ej = P.rowptr.copy(), P.col.copy(), P.val.copy(), Q.ei.copy(), Q.ej.copy()
    h = _compile(c, LR.ROW_BODIES[row][0], GL.EDGE_BODIES[edge], LR.RIDGE if with_ridge else None)
    before = _launches(c.core)
    L.check(c.core.lbfgsx_objective_bind_linear_graph(c.h, h, P.R, P.nnz, _vp(rp), _vp(col), _vp(val), 0, lanes, Q.E, _vp(ei),
                                                      _vp(ej), 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
    assert _launches(c.core) == before + BIND_LAUNCHES
    for a in (rp, col, ei, ej):  # the binding keeps its own copies
        a[:] = -5
    val[:] = 0
    assert oid.value == L.OBJ_BOUND
    lanes_used = lanes or LR.lanes_rule(P.R, P.nnz)
    info = _info(c)
    assert (info["R"], info["nnz"], info["L"], info["C"]) == (P.R, P.nnz, lanes_used, LR.C_DEFAULT)
    assert (info["nlong"] > 0) == Q.has_long()
    return oid.value, lanes_used, lambda x: Q.evaluate(x, lanes_used, row, edge, with_ridge)


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,name", CASES)
def test_eval_and_trial_statements_in_both_tile_orders(A, dtype, name):
    Q = _problem(name, dtype)
    n = Q.n
    per_eval = 3 if Q.has_long() else 2
    rng = np.random.default_rng(100 + n)
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
        for lanes in LANES[name]:
            for row, edge, with_ridge in BODIES:
                what = "%s lanes %d %s %s%s" % (name, lanes, row, edge, " +ridge" if with_ridge else "")
                oid, _, ref = _bind(c, Q, row, edge, with_ridge, lanes)
                fx, g2, x2 = _d(3)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
                assert _launches(c.core) == before + per_eval
                g_ref, terms = ref(xp)
                _bits(c.down(L.VEC_G), g_ref, what + ": g")
                _sum_ok(fx.value, terms, dt, what + ": f")
                _dot_ok(g2.value, g_ref, g_ref, dt, what + ": g.g")
                _dot_ok(x2.value, xp, xp, dt, what + ": x.x")
                g_ref, terms = ref(xt_ref)
                runs = []
                for k in range(2):
                    c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible; a gather of it would show
                    c.up(L.VEC_GT, stale)
                    fx, dg = _d(2)
                    before = _launches(c.core)
                    L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                    assert _launches(c.core) == before + per_eval
                    _bits(c.down(L.VEC_XT), xt_ref, "%s launch %d: x trial" % (what, k))
                    _bits(c.down(L.VEC_GT), g_ref, "%s launch %d: g trial" % (what, k))
                    runs.append((fx.value, dg.value))
                assert runs[0] == runs[1], what + ": f or g.d depends on the tile order"
                _sum_ok(runs[0][0], terms, dt, what + ": f trial")
                _dot_ok(runs[0][1], g_ref, d, dt, what + ": g.d")
                assert np.any(g_ref != 0)
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,name", CASES)
def test_b_eval_and_dg_maxstep_trial_statements(A, monkeypatch, dtype, name):
    """lbfgsx_b_eval, then the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d
    that lbfgsx_trial then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    Q = _problem(name, dtype)
    n = Q.n
    per_eval = 3 if Q.has_long() else 2
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for lanes in LANES[name]:
            for row, edge, with_ridge in BODIES:
                what = "%s lanes %d %s %s%s" % (name, lanes, row, edge, " +ridge" if with_ridge else "")
                oid, _, ref = _bind(c, Q, row, edge, with_ridge, lanes)
                for which, arr in ((L.VEC_X, x), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                    c.up(which, arr)
                fx, pg, x2 = _d(3)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
                assert _launches(c.core) == before + per_eval
                g_ref, terms = ref(x)
                _bits(c.down(L.VEC_G), g_ref, what + ": g")
                _sum_ok(fx.value, terms, dt, what + ": f")
                _dot_ok(x2.value, x, x, dt, what + ": x.x")
                assert pg.value == R.projg_norm_ref(x, g_ref, lb, ub), what
                c.up(L.VEC_G, g0)
                L.check(c.core.lbfgsx_ls_begin(c.h))
                c.up(L.VEC_XT, np.full(n, -77.0, dt))
                runs0, hits0 = _ahead(c)
                dg, sm = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
                assert _launches(c.core) == before + per_eval  # the first trial rides on the dg / max-step pass
                assert _ahead(c) == (runs0 + 1, hits0), what + ": the fused kernel did not run"
                g_ref, terms = ref(xt_ref)
                _bits(c.down(L.VEC_XT), xt_ref, what + ": x trial left by the fused pass")
                _bits(c.down(L.VEC_GT), g_ref, what + ": g trial left by the fused pass")
                fx, dgt = _d(2)
                before = _launches(c.core)
                L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
                assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)  # handed out ahead: no launch
                _bits(c.down(L.VEC_G), g0, what + ": g at xp is left alone")
                _dot_ok(dg.value, g0, d, dt, what + ": g.d")
                assert sm.value == R.step_max_ref(x, d, lb, ub), what
                _sum_ok(fx.value, terms, dt, what + ": f trial")
                _dot_ok(dgt.value, g_ref, d, dt, what + ": grad(x).d")


# ---------------------------------------------------------------- the topology
def _topologies_match(c, Q, lanes):
    P = Q.P
    info = _info(c)
    assert info["L"] == (lanes or LR.lanes_rule(P.R, P.nnz))
    colptr, trow, tpos = np.full(P.n + 1, 7, np.uint32), np.full(P.nnz, 7, np.int32), np.full(P.nnz, 7, np.uint32)
    long_col, long_chunk = np.full(info["nlong"], 7, np.int32), np.full(info["nlong"] + 1, 7, np.uint32)
    chunk = np.full((info["nchunks"], 2), 7, np.uint32)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, None, colptr.ctypes.data_as(u32p), trow.ctypes.data_as(i32p),
                                                      tpos.ctypes.data_as(u32p), long_col.ctypes.data_as(i32p),
                                                      long_chunk.ctypes.data_as(u32p), chunk.ctypes.data_as(u32p)))
    for got, want in zip((colptr, trow, tpos), P.topo):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    want = LR.chunk_table(P.topo[0])
    if info["nlong"] == 0:
        assert want[0].size == 0 and info["nchunks"] == 0
    else:
        for got, w in zip((long_col, long_chunk, chunk), want):
            assert got.dtype == w.dtype and np.array_equal(got, w)
    E = C.c_int64(-1)
    off, other, es = np.full(Q.n + 1, 7, np.uint32), np.full(2 * Q.E, 7, np.int32), np.full(2 * Q.E, 7, np.uint32)
    c.L.check(c.core.lbfgsx_objective_topology(c.h, C.byref(E), off.ctypes.data_as(u32p), other.ctypes.data_as(i32p),
                                               es.ctypes.data_as(u32p)))
    assert E.value == Q.E
    for got, want in zip((off, other, es), GR.incidence(Q.ei, Q.ej, Q.n)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["pair", "tiny", "random", "long"])
def test_both_topologies_are_the_lists_of_the_restatement(A, name):
    Q = _problem(name, O.F64)
    with Ctx(A, O.F64, Q.n) as c:
        for lanes in LANES[name]:
            _bind(c, Q, "hinge", "spring", False, lanes)
            _topologies_match(c, Q, lanes)


def test_matrix_and_edges_may_be_device_arrays(A):
    """matrix_on_device = 1 and edges_on_device = 1, together and one at a time: the same lists and the same gradient bits"""
    import torch
    Q = GL.Problem(LR.random_rows(200, 640, 9, 21, np.float64), *GR.random_multigraph(640, 8))
    P = Q.P
    with Ctx(A, O.F64, Q.n) as c:
        L = c.L
        x = np.random.default_rng(5).standard_normal(Q.n)
        c.up(L.VEC_X, x)
        oid, lanes, ref = _bind(c, Q, "cubic", "asym", True, 0)
        fx, g2, x2 = _d(3)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        want = (c.down(L.VEC_G).copy(), fx.value)
        _bits(want[0], ref(x)[0], "g against the restatement")
        host = (P.rowptr, P.col, P.val, Q.ei, Q.ej)
        dev = [torch.from_numpy(a.copy()).cuda() for a in host]
        torch.cuda.synchronize()
        h = _compile(c, LR.CUBIC, GL.ASYM_EDGE, LR.RIDGE)
        for m_dev, e_dev in ((1, 1), (1, 0), (0, 1)):
            ptrs, cs = _upload(c, Q)
            m = [C.c_void_p(t.data_ptr()) for t in dev[:3]] if m_dev else [_vp(a) for a in host[:3]]
            e = [C.c_void_p(t.data_ptr()) for t in dev[3:]] if e_dev else [_vp(a) for a in host[3:]]
            oid = C.c_int(-1)
            L.check(c.core.lbfgsx_objective_bind_linear_graph(c.h, h, P.R, P.nnz, m[0], m[1], m[2], m_dev, 0, Q.E, e[0], e[1], e_dev,
                                                              C.byref(ptrs), C.byref(cs), C.byref(oid)))
            _topologies_match(c, Q, 0)
            c.up(L.VEC_G, np.zeros(Q.n))
            L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
            _bits(c.down(L.VEC_G), want[0], "g from device arrays (matrix %d, edges %d)" % (m_dev, e_dev))
            assert fx.value == want[1]


def test_python_class_takes_numpy_arrays_and_device_tensors(A):
    """GraphLinearObjective with the matrix as numpy arrays and as torch tensors on the device: the same iterates, bit for bit"""
    import torch
    Q = GL.Problem(LR.random_rows(300, 80, 12, 33, np.float64), *GR.ring_chords(80))
    P = Q.P
    x0 = np.random.default_rng(6).standard_normal(Q.n)
    out = []
    for dev in (False, True):
        m = (P.rowptr, P.col, P.val)
        if dev:
            m = tuple(torch.from_numpy(a.copy()).cuda() for a in m)
        f = A.GraphLinearObjective(LR.HINGE, m, (Q.ei, Q.ej), GL.SPRING_EDGE, n=Q.n, coord_body=LR.RIDGE,
                                   data=(P.p0, None, Q.p2), scalars=(0.1,))
        assert f.on_device == dev
        s = A.LBFGSSolver(A.LBFGSParam(m=5, epsilon=0, epsilon_rel=0, max_iterations=8), linesearch=A.LS_MORE_THUENTE)
        x = x0.copy()
        niter, fx = s.minimize(f, x)
        out.append((niter, s.last.nfev, fx, x))
    assert out[0][:3] == out[1][:3] and out[0][0] == 8
    _bits(out[1][3], out[0][3], "x from device tensors")
    z = LR.row_sums(P.rowptr, P.col, P.val, x0, LR.lanes_rule(P.R, P.nnz))
    f0 = float(np.sum(LR.hinge(z, P.p0)[1]) + np.sum(LR.ridge(x0, 0.1)[1]) +
               np.sum(GR.spring_terms(x0, Q.ei.astype(np.int64), Q.ej.astype(np.int64), Q.p2)[1]))
    assert out[0][2] < f0  # it went down from the start value


# ---------------------------------------------------------------- rebinding
def test_rebinding_one_context_across_the_forms_leaks_no_list(A):
    """linear-graph -> linear -> graph -> linear-graph on one context: each evaluation is bit-equal to its own restatement, so
    neither list survives into a form that does not have it and neither is freed under a form that does"""
    Q = GL.Problem(LR.random_rows(150, 301, 10, 41, np.float64), *GR.random_multigraph(301, 9))
    Q2 = GL.Problem(LR.random_rows(90, 301, 14, 42, np.float64), *GR.ring_chords(301))  # another matrix and graph, the same n
    P = Q.P
    with Ctx(A, O.F64, Q.n) as c:
        L = c.L
        x = np.random.default_rng(8).standard_normal(Q.n)
        c.up(L.VEC_X, x)
        fx, g2, x2 = _d(3)

        def evaluate(oid, per_eval=2):
            c.up(L.VEC_G, np.full(Q.n, -77.0))
            before = _launches(c.core)
            L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
            assert _launches(c.core) == before + per_eval
            return c.down(L.VEC_G), fx.value

        oid, lanes, ref = _bind(c, Q, "cubic", "asym", True, 0)
        g, f = evaluate(oid)
        _bits(g, ref(x)[0], "linear-graph")
        _sum_ok(f, ref(x)[1], c.dt, "linear-graph: f")
        # the linear form alone, on the same matrix
        ptrs, cs = _upload(c, Q)
        hl, oid = C.c_void_p(), C.c_int(-1)
        log = C.create_string_buffer(8192)
        assert c.core.lbfgsx_objective_compile_linear(C.byref(hl), c.dtype, LR.RIDGE.encode(), LR.CUBIC.encode(), log, len(log)) == 0
        before = _launches(c.core)
        L.check(c.core.lbfgsx_objective_bind_linear(c.h, hl, P.R, P.nnz, _vp(P.rowptr), _vp(P.col), _vp(P.val), 0, 0, C.byref(ptrs),
                                                    C.byref(cs), C.byref(oid)))
        assert _launches(c.core) == before + LINEAR_LAUNCHES
        assert c.core.lbfgsx_objective_topology(c.h, None, None, None, None) == L.E_INVALID  # no graph list under this form
        g, f = evaluate(oid.value)
        g_lin, t_lin = P.evaluate(x, lanes, "cubic", True)
        _bits(g, g_lin, "linear after linear-graph")
        _sum_ok(f, t_lin, c.dt, "linear after linear-graph: f")
        # the graph form alone, on the same edges: the edge body reads p2, p3, c[4], c[5] as before
        hg = C.c_void_p()
        assert c.core.lbfgsx_objective_compile_graph(C.byref(hg), c.dtype, None, GL.ASYM_EDGE.encode(), log, len(log)) == 0
        before = _launches(c.core)
        L.check(c.core.lbfgsx_objective_bind_graph(c.h, hg, Q.E, Q.ei.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   Q.ej.ctypes.data_as(C.POINTER(C.c_int32)), 0, C.byref(ptrs), C.byref(cs),
                                                   C.byref(oid)))
        assert _launches(c.core) == before + GRAPH_LAUNCHES
        assert c.core.lbfgsx_objective_linear_topology(c.h, None, None, None, None, None, None, None) == L.E_INVALID
        g, f = evaluate(oid.value, 1)
        tg, ev = GL.edge_terms("asym", x, Q.ei.astype(np.int64), Q.ej.astype(np.int64), Q.p2, Q.p3)
        _bits(g, GR.graph_grad(tg, Q.ei, Q.ej, Q.n), "graph after linear")
        _sum_ok(f, ev, c.dt, "graph after linear: f")
        # and the combined form again, with another matrix and another graph
        oid, lanes, ref = _bind(c, Q2, "hinge", "spring", False, 4)
        g, f = evaluate(oid)
        _bits(g, ref(x)[0], "linear-graph after graph")
        _sum_ok(f, ref(x)[1], c.dt, "linear-graph after graph: f")
        _topologies_match(c, Q2, 4)
        for h in (hl, hg):
            c.core.lbfgsx_objective_destroy(h)


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "graph_linear_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


QUARTIC_EDGE = """const T d = x[0] - x[1];
const T q = c[1] * ((d * d) * d);
g[0] = q;
g[1] = T(0) - q;
return T(0.25) * (q * d);"""
SMOOTH_EDGE = """const T d = x[0] - x[1];
const T q = c[1] * d;
g[0] = q;
g[1] = T(0) - q;
return T(0.5) * (q * d);"""


def _probe_instance(A, solver, R_, n, k):
    """tests/cpp/graph_linear_probe.cpp: the matrix, the graph, the per-row data and start(), operation for operation"""
    r, j = np.arange(R_)[:, None], np.arange(k["per"])[None, :]
    col = ((7 * r + 3 * j * j + j) % n).reshape(-1)
    val = (((31 * r + 17 * j) % 13 - 6) / 4.0).reshape(-1)
    rowptr = np.arange(0, R_ * k["per"] + 1, k["per"])
    r = r.reshape(-1)
    y, b = np.where((5 * r) % 3 == 0, -1.0, 1.0), ((11 * r) % 7 - 3) / 2.0
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    x0 = k["amp"] * ((0.5 - t) * (1.0 + t))
    edges = GR.ring_chords(n)
    if solver == "lbfgs":
        return A.GraphLinearObjective(LR.HINGE, (rowptr, col, val), edges, QUARTIC_EDGE, n=n, coord_body=LR.RIDGE, data=(y,),
                                      scalars=(k["c0"], k["c1"])), x0
    return A.GraphLinearObjective(LR.SQUARE, (rowptr, col, val), edges, SMOOTH_EDGE, n=n, data=(b,), scalars=(k["c0"], k["c1"])), x0


def test_the_probe_holds_the_bodies_of_this_test():
    src = open(os.path.join(ROOT, "tests", "cpp", "graph_linear_probe.cpp")).read()
    for body in (LR.HINGE, LR.RIDGE, LR.SQUARE, QUARTIC_EDGE, SMOOTH_EDGE):
        for line in body.strip().splitlines():
            assert '"%s' % line in src, line


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%dx%d" % (i["solver"], i["R"], i["n"]))
def test_graph_linear_models_follow_the_reference(A, inst):
    n, tol = inst["n"], _golden()["tolerance"]
    assert inst["iterations"] >= 8
    f, x0 = _probe_instance(A, inst["solver"], inst["R"], n, _golden()["constants"])
    lb, ub = np.zeros(n), np.full(n, np.inf)
    assert np.any(x0 < lb)  # bounds are active at the projected start
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


def test_cpp_graph_linear_objective_follows_the_reference(tmp_path):
    """tests/cpp/graph_linear_probe.cpp with GraphLinearObjective<double> in place of the functor, built with g++ against
    include/"""
    exe = str(tmp_path / "graph_linear_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DGRAPH_LINEAR_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "graph_linear_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    tol = _golden()["tolerance"]
    for shape in sorted({(i["R"], i["n"]) for i in insts}):
        mine = [i for i in insts if (i["R"], i["n"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe, str(shape[0]), str(shape[1]), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=300)
        assert out.returncode == 0 and "GRAPH LINEAR PROBE OK" in out.stdout, out.stdout[-2000:]
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
                assert np.abs(x - x_ref).max() <= tol and abs(fx - inst["f"][k - 1]) <= tol, (inst["solver"], shape, k)


# ---------------------------------------------------------------- convergence
def _regression(R_, n, seed, per_row=8):
    """R_ x n with per_row entries per row, as CSR and dense"""
    rng = np.random.default_rng(seed)
    rows = [sorted(rng.choice(np.arange(n), per_row, replace=False).tolist()) for _ in range(R_)]
    rowptr = np.arange(0, R_ * per_row + 1, per_row, dtype=np.int32)
    col = np.asarray(rows, np.int32).reshape(-1)
    val = rng.standard_normal(col.size)
    dense = np.zeros((R_, n))
    np.add.at(dense, (np.repeat(np.arange(R_), per_row), col), val)
    return rng, (rowptr, col, val), dense


def _laplacian(ei, ej, n):
    Lap = np.zeros((n, n))
    for i, j in zip(ei, ej):
        Lap[i, i] += 1.0
        Lap[j, j] += 1.0
        Lap[i, j] -= 1.0
        Lap[j, i] -= 1.0
    return Lap


def _model_bytes(core):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), 0) == 0
    return cnt[3]


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_laplacian_regularised_least_squares_converges_to_the_normal_equations(A, solver):
    """f = 1/2 |A x - b|^2 + lam/2 sum over edges of (x_i - x_j)^2, A 60 x 90 (under-determined: the graph term makes the
    problem definite): g = H (x - x*) with H = A^T A + lam Lap, so |x - x*| <= |g| / lambda_min(H), and the solver stops at
    |g| <= eps max(1, |x|) (a factor 2 for the other summation order): the tolerance is computed here, the way
    test_least_squares_converges_to_lstsq of the linear form computes its own.  The ring with chords is connected, so Lap's
    null space is the constant vector, which A does not annihilate: H is positive definite."""
    core, _ = A.load()
    R_, n, eps, lam = 60, 90, 1e-6, 0.7
    rng, m, dense = _regression(R_, n, 81, per_row=6)
    b = dense @ rng.standard_normal(n) + 0.1 * rng.standard_normal(R_)
    ei, ej = GR.ring_chords(n)
    E = ei.size
    H = dense.T @ dense + lam * _laplacian(ei, ej, n)
    x_star = np.linalg.solve(H, dense.T @ b)
    lmin = float(np.linalg.eigvalsh(H)[0])
    assert lmin > 1e-3
    f = A.GraphLinearObjective(LR.SQUARE, m, (ei, ej), SMOOTH_EDGE, n=n, data=(b,), scalars=(0.0, lam))
    x = np.zeros(n)
    cap = 3000
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        before = _model_bytes(core)
        niter, fx = s.minimize(f, x)
        # the byte model (launch_args.hpp): the linear form's terms plus the graph form's list terms; no column is long here.
        # The first evaluation is lbfgsx_eval (1 vector gathered), every other one a trial (2: xp and d), which also reads xp
        # and d, writes x and grad and reads the data array
        lin = lambda vg: (f.R + 1) * 4 + (n + 1) * 4 + 2 * f.nnz * 4 + 2 * f.nnz * 8 + f.nnz * 8 * (vg + 1) + 4 * f.R * 8
        gra = lambda vg: (n + 1) * 4 + 2 * E * 8 + 2 * E * 8 * vg
        assert _model_bytes(core) - before == lin(1) + gra(1) + (s.last.nfev - 1) * (n * 8 * (4 + len(f.data)) + lin(2) + gra(2))
    else:
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        niter, fx = s.minimize(f, x, np.full(n, -50.0), np.full(n, 50.0))
        assert np.abs(x).max() < 50.0  # no bound is active: the projected gradient is the gradient
    assert 0 < niter < cap
    g = H @ x - dense.T @ b
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    gnorm = float(np.linalg.norm(g))
    measure = gnorm if solver == "lbfgs" else float(np.abs(g).max())
    tol = 2.0 * bound * (1.0 if solver == "lbfgs" else np.sqrt(n)) / lmin  # the inf-norm rule bounds |g|_2 by sqrt(n) times it
    err = float(np.linalg.norm(x - x_star))
    print("%s: niter %d nfev %d fx %.12g |g| %.3g (bound %.3g) lambda_min %.3g |x - x*| %.3g (tolerance %.3g)"
          % (solver, niter, s.last.nfev, fx, gnorm, bound, lmin, err, tol))
    assert measure <= 2.0 * bound
    assert err <= tol


def test_lbfgsb_solve_takes_the_fused_dg_maxstep_trial_with_active_bounds(A):
    """non-negative least squares with a smoothness term: bounds active at the start and at the end; every iteration's first
    trial is handed out by the dg / max-step pass"""
    core, _ = A.load()
    R_, n, iters, lam = 300, 40, 15, 0.3
    rng, m, dense = _regression(R_, n, 79, per_row=5)
    b = dense @ rng.standard_normal(n)
    ei, ej = GR.ring_chords(n)
    f = A.GraphLinearObjective(LR.SQUARE, m, (ei, ej), SMOOTH_EDGE, n=n, data=(b,), scalars=(0.0, lam))
    s = A.LBFGSBSolver(A.LBFGSBParam(m=6, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
    s.prepare(n)
    lb, ub = np.zeros(n), np.full(n, np.inf)
    x = np.zeros(n)
    f0 = 0.5 * float(b @ b)
    niter, fx = s.minimize(f, x, lb, ub)
    ahead = (C.c_int64 * 2)()
    assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
    print(niter, s.last.nfev, fx, f0, ahead[0], ahead[1])
    assert niter > 0 and ahead[0] > 0 and ahead[1] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert fx < f0 and (x >= 0).all() and (x == 0).any() and (x > 0).any()
    r = dense @ x - b
    d = x[ei] - x[ej]
    assert abs(fx - (0.5 * float(r @ r) + 0.5 * lam * float(d @ d))) <= 1e-10 * max(1.0, fx)


# ---------------------------------------------------------------- refusals
def _nothing_bound(c):
    fx, g2, x2 = _d(3)
    before = _launches(c.core)
    assert c.core.lbfgsx_eval(c.h, c.L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
    assert _launches(c.core) == before
    assert c.core.lbfgsx_objective_linear_topology(c.h, None, None, None, None, None, None, None) == c.L.E_INVALID
    assert c.core.lbfgsx_objective_topology(c.h, None, None, None, None) == c.L.E_INVALID


def test_offending_edges_and_matrices_are_refused_by_value_and_nothing_is_evaluated(A):
    n = 6
    good_m = ([0, 2, 2, 5], [0, 3, 5, 1, 4], [1.0, 2.0, 3.0, 4.0, 5.0])  # R = 3, nnz = 5
    good_e = ([0, 1, 5], [1, 2, 0])
    with Ctx(A, O.F64, n) as c:
        L = c.L
        h = _compile(c, LR.HINGE, GL.SPRING_EDGE)

        def bind(m=good_m, e=good_e, R_=None, nnz=None, E=None, handle=h, lanes=0, oid=None):
            rp, col, val = np.asarray(m[0], np.int32), np.asarray(m[1], np.int32), np.asarray(m[2], np.float64)
            ei, ej = np.asarray(e[0], np.int32), np.asarray(e[1], np.int32)
            return c.core.lbfgsx_objective_bind_linear_graph(c.h, handle, len(m[0]) - 1 if R_ is None else R_,
                                                             len(m[1]) if nnz is None else nnz, _vp(rp), _vp(col), _vp(val), 0, lanes,
                                                             len(e[0]) if E is None else E, _vp(ei), _vp(ej), 0, None, None, oid)
        # an offending list: the edges are validated first (1 launch), the matrix after the edges' 5
        cases = [("self-loop", dict(e=([0, 2, 5], [1, 2, 0])), "edge e = 1 is (i = 2, j = 2) with n = 6", "1 of the E = 3 edges", 1),
                 ("node = n", dict(e=([0, 1, 6], [1, 2, 0])), "edge e = 2 is (i = 6, j = 0) with n = 6", "1 of the E = 3 edges", 1),
                 ("node = -1", dict(e=([0, 1, 5], [-1, 2, 9])), "edge e = 0 is (i = 0, j = -1) with n = 6", "2 of the E = 3 edges", 1),
                 ("rowptr decreases", dict(m=([0, 3, 2, 5], good_m[1], good_m[2])), "rowptr[2] = 2 with R = 3, nnz = 5",
                  "1 of the 9 positions", GRAPH_LAUNCHES + 1),
                 ("col = n", dict(m=(good_m[0], [0, 3, 5, 6, 4], good_m[2])), "col[3] = 6 with n = 6", "1 of the 9 positions",
                  GRAPH_LAUNCHES + 1),
                 ("both offend: the edge is named", dict(e=([0, 1, 5], [1, 1, 0]), m=(good_m[0], [0, 7, 5, 1, 9], good_m[2])),
                  "edge e = 1 is (i = 1, j = 1) with n = 6", "1 of the E = 3 edges", 1)]
        for name, kw, what, count, launches in cases:
            assert bind() == 0  # something is bound before each refusal
            before = _launches(c.core)
            rc = bind(oid=C.byref(C.c_int(-1)), **kw)
            assert rc == L.E_INVALID and what in L.last_error() and count in L.last_error(), L.last_error()
            assert _launches(c.core) == before + launches, name
            _nothing_bound(c)
        lim = 2 ** 31
        for kw, what in ((dict(E=0), "E = 0"), (dict(E=-1), "E = -1"), (dict(E=lim), "E = 2147483648 exceeds 2^31 - 1"),
                         (dict(R_=0), "R = 0, nnz = 5"), (dict(nnz=0), "R = 3, nnz = 0"),
                         (dict(R_=lim), "R = 2147483648 exceeds 2^31 - 1"), (dict(nnz=lim), "nnz = 2147483648 exceeds 2^31 - 1"),
                         (dict(lanes=3), "lanes = 3"), (dict(lanes=128), "lanes = 128")):
            assert bind() == 0
            before = _launches(c.core)
            assert bind(**kw) == L.E_INVALID and what in L.last_error(), L.last_error()
            assert L.last_error().startswith("graph-regularised linear-model objective: ")
            assert _launches(c.core) == before
            _nothing_bound(c)
        assert bind() == 0
        fl = A.LinearObjective(LR.HINGE, good_m, n)
        fg = A.GraphObjective(GL.SPRING_EDGE, good_e)
        for f, name in ((fl, "linear-model objective"), (fg, "graph objective")):
            assert bind(handle=f.compile()) == L.E_INVALID
            assert "the handle is a %s, not a graph-regularised linear-model objective" % name in L.last_error()
            _nothing_bound(c)
            assert bind() == 0
        f32 = A.GraphLinearObjective(LR.HINGE, good_m, good_e, GL.SPRING_EDGE, n=n)
        assert bind(handle=f32.compile(np.float32)) == L.E_INVALID and "the other dtype" in L.last_error()
        _nothing_bound(c)
        # the other bind calls refuse the handle
        said = "a graph-regularised linear-model objective is bound with its matrix and edges: lbfgsx_objective_bind_linear_graph"
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID and said in L.last_error()
        rp, col, val = (np.asarray(a, t) for a, t in zip(good_m, (np.int32, np.int32, np.float64)))
        assert c.core.lbfgsx_objective_bind_linear(c.h, h, 3, 5, _vp(rp), _vp(col), _vp(val), 0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a graph-regularised linear-model objective, not a linear-model objective" in L.last_error()
        i32p = C.POINTER(C.c_int32)
        e0, e1 = np.zeros(3, np.int32).ctypes.data_as(i32p), np.ones(3, np.int32).ctypes.data_as(i32p)
        assert c.core.lbfgsx_objective_bind_graph(c.h, h, 3, e0, e1, 0, None, None, None) == L.E_INVALID
        assert "the handle is a graph-regularised linear-model objective, not a graph objective" in L.last_error()
        assert c.core.lbfgsx_objective_bind_mesh(c.h, h, 1, e0, 0, None, None, None) == L.E_INVALID
        assert "not a mesh objective" in L.last_error()
        assert c.core.lbfgsx_objective_bind_grid(c.h, h, 2, 3, None, None, None) == L.E_INVALID
        assert "not a grid objective" in L.last_error()
        _nothing_bound(c)
        oid = C.c_int(-1)
        assert bind(oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
    # through the solver: ValueError with the position named
    for m, e, what in ((([0, 1, 2], [0, 6], [1.0, 1.0]), good_e, "col\\[1\\] = 6 with n = 6"),
                       (good_m, ([0, 3], [1, 3]), "edge e = 1 is \\(i = 3, j = 3\\) with n = 6")):
        with pytest.raises(ValueError, match=what):
            A.LBFGSSolver(A.LBFGSParam()).minimize(
                A.GraphLinearObjective(LR.HINGE, m, e, GL.SPRING_EDGE, n=6, data=(np.ones(len(m[0]) - 1), None, np.ones(len(e[0])))),
                np.zeros(6))


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    Q = GL.Problem(LR.random_rows(50, 64, 6, 3, np.float64), *GR.ring_chords(64))
    f = A.GraphLinearObjective(LR.HINGE, (Q.P.rowptr, Q.P.col, Q.P.val), (Q.ei, Q.ej), GL.SPRING_EDGE, n=64, coord_body=LR.RIDGE,
                               data=(Q.P.p0, None, Q.p2), scalars=(0.1,))
    s = A.LBFGSSolver(A.LBFGSParam())
    s.set_recursion(L.RECURSION_GRAM_SPACE)
    with pytest.raises(ValueError, match="TermObjective runs with the vector recursion"):
        s.minimize(f, np.zeros(64))
    s2 = A.LBFGSSolver(A.LBFGSParam())
    s2.set_devices([0, 0])
    with pytest.raises(ValueError, match="row-sharded run needs a built-in objective"):
        s2.minimize(f, np.zeros(64))
    batch = B.LockstepBatch(A.LBFGSParam(m=3, max_iterations=3), 64, 2, dtype=np.float64)
    try:
        with pytest.raises(TypeError, match="fn must be callable"):
            batch.minimize_fn(f, np.zeros((2, 64)))
    finally:
        batch.close()
