"""-m gpu: linear-model objectives (lbfgspp_amd.LinearObjective, csrc/linear_kernels.cuh, csrc/linear_topology.hip) on the
device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders, a stale trial vector in
    place), lbfgsx_b_eval and lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/linear_ref.py -- gradient and
    written x bit for bit, f and the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly equal
    -- for two row bodies with and without a ridge, on the 1 x 1 matrix, a 3 x 5 one with an empty row, an empty column and a
    duplicate entry, random rows with every lane count, many columns, and long columns; all bound one after another to one
    context (the matrix is rebuilt at every bind).  The launches are counted: 6 per bind, 2 per evaluation, 3 with a long
    column, none for a trial handed out ahead;
  * lbfgsx_objective_linear_topology is the transposed list, L and chunk table of the restatement; a matrix given as device
    tensors gives the same bits;
  * the squared hinge with a ridge and non-negative least squares follow the reference (tests/golden/linear_golden.json), from
    Python and C++;
  * logistic regression with an intercept and least squares converge under both solvers; refusals by value."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import linear_ref as LR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
PACK = {O.F64: 2, O.F32: 4}  # W: the coordinates a thread owns (the values of a 16-byte pack)
BIND_LAUNCHES = 6            # validation, expansion, sort, column offsets, entries, long-column search
BODIES = [("cubic", False), ("cubic", True), ("hinge", False), ("hinge", True)]


def _wide_n(dtype):
    """more than one block's trial tiles plus a ragged tail: the mesh test's largest size"""
    W = PACK[dtype]
    return 5 * 256 * LR.TRIAL_U * W + W + 1


def _problem(name, dtype):
    dt = NPDT[dtype]
    if name == "single":
        return LR.single(dt)
    if name == "tiny":
        return LR.tiny(dt)
    if name == "random":
        return LR.random_rows(700, 1031, 40, 7, dt)
    if name == "wide":
        return LR.random_rows(300, _wide_n(dtype), 12, 8, dt)
    if name == "tile":  # one coordinate past one trial tile of the column pass, R < n: the grid is chosen by n
        return LR.random_rows(200, 256 * LR.TRIAL_U * PACK[dtype] + 1, 12, 9, dt)
    return LR.long_columns(dt)


# single: n = 1, no whole pack; tiny (n = 5, R = 3) and long (n = 37, R = 9000): one coordinate past the last pack, the grid
# chosen by n and by R
LANES = {"single": (0, 2), "tiny": (0, 4), "random": (0, 1, 2, 8, 64), "wide": (0,), "tile": (0,), "long": (0,)}
CASES = [pytest.param(dt, name, id="%s-%s" % ("f64" if dt == O.F64 else "f32", name))
         for dt in (O.F64, O.F32) for name in ("single", "tiny", "random", "wide", "tile", "long")]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled = {}


def _compile(c, row, coord=None):
    key = (row, coord, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_linear(C.byref(h), c.dtype, coord.encode() if coord else None, row.encode(), log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        _compiled[key] = h
    return _compiled[key]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _info(c):
    info = (C.c_int64 * 8)()
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, C.byref(info), None, None, None, None, None, None))
    return dict(zip(("R", "nnz", "L", "C", "nlong", "nchunks"), list(info)[:6]))


def _bind(c, P, row, with_ridge, lanes):
    """compiles (once per process) and binds the row body (and RIDGE) with P's per-row data; returns (id, L, x -> (g, terms))"""
    L = c.L
    dev = C.c_void_p()
    L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, _vp(P.p0), P.R, C.byref(dev)))
    ptrs = (C.c_void_p * 4)()
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(P.c0, *([0.0] * 7))
    oid = C.c_int(-1)
    rp, col, val = P.rowptr.copy(), P.col.copy(), P.val.copy()
    h = _compile(c, LR.ROW_BODIES[row][0], LR.RIDGE if with_ridge else None)
    before = _launches(c.core)
    L.check(c.core.lbfgsx_objective_bind_linear(c.h, h, P.R, P.nnz, _vp(rp), _vp(col), _vp(val), 0, lanes, C.byref(ptrs),
                                                C.byref(cs), C.byref(oid)))
    assert _launches(c.core) == before + BIND_LAUNCHES
    rp[:] = -5  # the binding keeps its own copies
    col[:] = -5
    val[:] = 0
    assert oid.value == L.OBJ_BOUND
    lanes_used = lanes or LR.lanes_rule(P.R, P.nnz)
    info = _info(c)
    assert (info["R"], info["nnz"], info["L"], info["C"]) == (P.R, P.nnz, lanes_used, LR.C_DEFAULT)
    assert (info["nlong"] > 0) == P.has_long()
    return oid.value, lanes_used, lambda x: P.evaluate(x, lanes_used, row, with_ridge)


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,name", CASES)
def test_eval_and_trial_statements_in_both_tile_orders(A, dtype, name):
    P = _problem(name, dtype)
    n = P.n
    per_eval = 3 if P.has_long() else 2
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
            for row, with_ridge in BODIES:
                what = "%s lanes %d %s%s" % (name, lanes, row, "+ridge" if with_ridge else "")
                oid, _, ref = _bind(c, P, row, with_ridge, lanes)
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
                assert P.nnz < 100 or np.any(g_ref != 0)
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,name", CASES)
def test_b_eval_and_dg_maxstep_trial_statements(A, monkeypatch, dtype, name):
    """lbfgsx_b_eval, then the fused first trial of L-BFGS-B: g.d and step_max, and the trial point, its gradient, f and grad.d
    that lbfgsx_trial then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    P = _problem(name, dtype)
    n = P.n
    per_eval = 3 if P.has_long() else 2
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for lanes in LANES[name]:
            for row, with_ridge in BODIES:
                what = "%s lanes %d %s%s" % (name, lanes, row, "+ridge" if with_ridge else "")
                oid, _, ref = _bind(c, P, row, with_ridge, lanes)
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
def _read_topology(c, P):
    info = _info(c)
    colptr, trow, tpos = np.full(P.n + 1, 7, np.uint32), np.full(P.nnz, 7, np.int32), np.full(P.nnz, 7, np.uint32)
    long_col, long_chunk = np.full(info["nlong"], 7, np.int32), np.full(info["nlong"] + 1, 7, np.uint32)
    chunk = np.full((info["nchunks"], 2), 7, np.uint32)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, None, colptr.ctypes.data_as(u32p), trow.ctypes.data_as(i32p),
                                                      tpos.ctypes.data_as(u32p), long_col.ctypes.data_as(i32p),
                                                      long_chunk.ctypes.data_as(u32p), chunk.ctypes.data_as(u32p)))
    return info, (colptr, trow, tpos), (long_col, long_chunk, chunk)


def _topology_matches(c, P, lanes):
    info, topo, table = _read_topology(c, P)
    assert info["L"] == (lanes or LR.lanes_rule(P.R, P.nnz))
    for got, want in zip(topo, P.topo):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    want = LR.chunk_table(P.topo[0])
    if info["nlong"] == 0:
        assert want[0].size == 0 and info["nchunks"] == 0
    else:
        for got, w in zip(table, want):
            assert got.dtype == w.dtype and np.array_equal(got, w)


@pytest.mark.parametrize("name", ["single", "tiny", "random", "wide", "long"])
def test_topology_is_the_transposed_list_of_the_restatement(A, name):
    P = _problem(name, O.F64)
    with Ctx(A, O.F64, P.n) as c:
        for lanes in LANES[name]:
            _bind(c, P, "hinge", False, lanes)
            _topology_matches(c, P, lanes)


def test_matrix_arrays_may_be_device_arrays(A):
    """matrix_on_device = 1: the same list and the same gradient bits from device copies of the three arrays (here: three of
    the context's own data buffers, which hold the int32 words as raw bytes)"""
    P = LR.random_rows(200, 640, 9, 21, np.float32)  # f32: an element of a data buffer is 4 bytes, as an index
    with Ctx(A, O.F32, P.n) as c:
        L = c.L
        x = np.random.default_rng(5).standard_normal(P.n).astype(np.float32)
        c.up(L.VEC_X, x)
        oid, lanes, ref = _bind(c, P, "cubic", True, 0)
        fx, g2, x2 = _d(3)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        want = (c.down(L.VEC_G).copy(), fx.value)
        dev = [C.c_void_p() for _ in range(4)]
        for slot, arr in ((0, P.p0), (1, P.rowptr), (2, P.col), (3, P.val)):
            L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, _vp(arr), arr.size, C.byref(dev[slot])))
        ptrs = (C.c_void_p * 4)()
        ptrs[0] = dev[0].value
        cs = (C.c_double * 8)(P.c0, *([0.0] * 7))
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind_linear(c.h, _compile(c, LR.CUBIC, LR.RIDGE), P.R, P.nnz, dev[1], dev[2], dev[3], 1, 0,
                                                    C.byref(ptrs), C.byref(cs), C.byref(oid)))
        _topology_matches(c, P, 0)
        L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
        _bits(c.down(L.VEC_G), want[0], "g from the device arrays")
        _bits(want[0], ref(x)[0], "g against the restatement")
        assert fx.value == want[1]


def test_python_class_takes_numpy_arrays_and_device_tensors(A):
    """LinearObjective with the matrix as numpy arrays and as torch tensors on the device: the same iterates, bit for bit"""
    import torch
    P = LR.random_rows(300, 80, 12, 33, np.float64)
    lam = 0.1
    x0 = np.random.default_rng(6).standard_normal(P.n)
    out = []
    for dev in (False, True):
        m = (P.rowptr, P.col, P.val)
        if dev:
            m = tuple(torch.from_numpy(a.copy()).cuda() for a in m)
        f = A.LinearObjective(LR.HINGE, m, P.n, coord_body=LR.RIDGE, data=(P.p0,), scalars=(lam,))
        assert f.on_device == dev
        s = A.LBFGSSolver(A.LBFGSParam(m=5, epsilon=0, epsilon_rel=0, max_iterations=8), linesearch=A.LS_MORE_THUENTE)
        x = x0.copy()
        niter, fx = s.minimize(f, x)
        out.append((niter, s.last.nfev, fx, x))
    assert out[0][:3] == out[1][:3] and out[0][0] == 8
    _bits(out[1][3], out[0][3], "x from device tensors")
    z = LR.row_sums(P.rowptr, P.col, P.val, x0, LR.lanes_rule(P.R, P.nnz))
    f0 = float(np.sum(LR.hinge(z, P.p0)[1]) + np.sum(LR.ridge(x0, lam)[1]))
    assert out[0][2] < f0  # it went down from the start value


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "linear_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


def _probe_instance(A, solver, R_, n, k):
    """tests/cpp/linear_probe.cpp: the matrix, the per-row data and start(), operation for operation"""
    r, j = np.arange(R_)[:, None], np.arange(k["per"])[None, :]
    col = ((7 * r + 3 * j * j + j) % n).reshape(-1)
    val = (((31 * r + 17 * j) % 13 - 6) / 4.0).reshape(-1)
    rowptr = np.arange(0, R_ * k["per"] + 1, k["per"])
    r = r.reshape(-1)
    y, b = np.where((5 * r) % 3 == 0, -1.0, 1.0), ((11 * r) % 7 - 3) / 2.0
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    x0 = k["amp"] * ((0.5 - t) * (1.0 + t))
    if solver == "lbfgs":
        return A.LinearObjective(LR.HINGE, (rowptr, col, val), n, coord_body=LR.RIDGE, data=(y,), scalars=(k["c0"],)), x0
    return A.LinearObjective(LR.SQUARE, (rowptr, col, val), n, data=(b,)), x0


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%dx%d" % (i["solver"], i["R"], i["n"]))
def test_linear_models_follow_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
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


def test_cpp_linear_objective_follows_the_reference(tmp_path):
    """tests/cpp/linear_probe.cpp with LinearObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "linear_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DLINEAR_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "linear_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["R"], i["n"]) for i in insts}):
        mine = [i for i in insts if (i["R"], i["n"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe, str(shape[0]), str(shape[1]), str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=300)
        assert out.returncode == 0 and "LINEAR PROBE OK" in out.stdout, out.stdout[-2000:]
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
def _regression(R_, n, seed, per_row=8):
    """R_ x n with a dense intercept column 0 and per_row other entries per row"""
    rng = np.random.default_rng(seed)
    rows = [[0] + sorted(rng.choice(np.arange(1, n), per_row, replace=False).tolist()) for _ in range(R_)]
    rowptr = np.arange(0, R_ * (per_row + 1) + 1, per_row + 1, dtype=np.int32)
    col = np.asarray(rows, np.int32).reshape(-1)
    val = rng.standard_normal(col.size)
    val[rowptr[:-1]] = 1.0
    dense = np.zeros((R_, n))
    np.add.at(dense, (np.repeat(np.arange(R_), per_row + 1), col), val)
    return rng, (rowptr, col, val), dense


def _model_bytes(core):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), 0) == 0
    return cnt[3]


def _solve(A, solver, f, n, eps, cap=3000):
    x = np.zeros(n)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        core, _ = A.load()
        before = _model_bytes(core)
        niter, fx = s.minimize(f, x)
        # the byte model (launch_args.hpp).  An evaluation of a linear-model objective: the offsets of both passes, their
        # indices and values, the gathered values (vg vectors in the row pass, w in the column pass), w and v written and read;
        # no column is long here.  A trial launch also reads xp and d, writes x and grad and reads the data arrays.  The first
        # evaluation is lbfgsx_eval (vg = 1), every other one a trial (vg = 2: xp and d)
        assert f.R <= LR.C_DEFAULT
        lin = lambda vg: (f.R + 1) * 4 + (n + 1) * 4 + 2 * f.nnz * 4 + 2 * f.nnz * 8 + f.nnz * 8 * (vg + 1) + 4 * f.R * 8
        assert _model_bytes(core) - before == lin(1) + (s.last.nfev - 1) * (n * 8 * (4 + len(f.data)) + lin(2))
    else:
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        niter, fx = s.minimize(f, x, np.full(n, -50.0), np.full(n, 50.0))
        assert np.abs(x).max() < 50.0  # no bound is active: the projected gradient is the gradient
    assert 0 < niter < cap
    return x, niter, fx, s.last.nfev


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_logistic_regression_with_an_intercept_converges(A, solver):
    """f = (1/R) sum log(1 + exp(-y_r z_r)) + lam/2 |x|^2, 2000 x 50 with an intercept column.  At the returned x the float64
    numpy gradient (np.logaddexp) meets the solver's own stopping rule with a factor 2: ||g|| <= 2 eps max(1, ||x||).  The
    device and numpy gradients differ by rounding (2000 terms of size <= 1/R each: about 1e-15), orders of magnitude below
    eps = 1e-6, so the factor cannot hide a wrong gradient"""
    R_, n, eps, lam = 2000, 50, 1e-6, 1e-3
    rng, m, dense = _regression(R_, n, 77)
    y = np.where(dense @ rng.standard_normal(n) + 0.5 * rng.standard_normal(R_) > 0, 1.0, -1.0)
    body = LR.LOGISTIC.replace("dz = T(0) - p0[r] * s;", "dz = c[1] * (T(0) - p0[r] * s);").replace(
        "return (m > T(0) ? T(0) : T(0) - m) + log1p(e);", "return c[1] * ((m > T(0) ? T(0) : T(0) - m) + log1p(e));")
    assert body.count("c[1]") == 2
    f = A.LinearObjective(body, m, n, coord_body=LR.RIDGE, data=(y,), scalars=(lam, 1.0 / R_))
    x, niter, fx, nfev = _solve(A, solver, f, n, eps)
    marg = y * (dense @ x)
    g = dense.T @ (-y * np.exp(-np.logaddexp(0.0, marg))) / R_ + lam * x
    f_np = float(np.mean(np.logaddexp(0.0, -marg)) + 0.5 * lam * (x @ x))
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    measure = float(np.linalg.norm(g)) if solver == "lbfgs" else float(np.abs(g).max())
    print("%s: niter %d nfev %d fx %.12g (numpy %.12g) stopping measure %.3g (bound %.3g)" % (solver, niter, nfev, fx, f_np, measure, bound))
    assert measure <= 2.0 * bound
    assert abs(fx - f_np) <= 1e-12 * max(1.0, abs(f_np)) * 10
    assert x[0] != 0  # the intercept moved


@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_least_squares_converges_to_lstsq(A, solver):
    """f = 1/2 |A x - b|^2: g = A^T A (x - x*), so |x - x*| <= |g| / sigma_min^2, and the solver stops at
    |g| <= eps max(1, |x|) (a factor 2 for the other summation order, as above): the tolerance is computed here.
    eps = 1e-6, the logistic test's: a step that takes |g| from eps |x| to zero lowers f by about (eps |x|)^2 / sigma_min^2,
    which has to stay well above the spacing of f's values, 2^-52 f(x*), for a line search to see it; at eps = 1e-8 it does
    not (f(x*) is the noise's 1/2 |r|^2)"""
    R_, n, eps = 400, 30, 1e-6
    rng, m, dense = _regression(R_, n, 78, per_row=6)
    b = dense @ rng.standard_normal(n) + 0.1 * rng.standard_normal(R_)
    x_star = np.linalg.lstsq(dense, b, rcond=None)[0]
    smin = float(np.linalg.svd(dense, compute_uv=False)[-1])
    f = A.LinearObjective(LR.SQUARE, m, n, data=(b,))
    x, niter, fx, nfev = _solve(A, solver, f, n, eps)
    g = dense.T @ (dense @ x - b)
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    gnorm = float(np.linalg.norm(g))
    measure = gnorm if solver == "lbfgs" else float(np.abs(g).max())
    tol = 2.0 * bound * (1.0 if solver == "lbfgs" else np.sqrt(n)) / smin ** 2  # the inf-norm rule bounds |g|_2 by sqrt(n) times it
    err = float(np.linalg.norm(x - x_star))
    print("%s: niter %d nfev %d fx %.12g |g| %.3g (bound %.3g) sigma_min %.3g |x - x*| %.3g (tolerance %.3g)"
          % (solver, niter, nfev, fx, gnorm, bound, smin, err, tol))
    assert measure <= 2.0 * bound
    assert err <= tol


def test_lbfgsb_solve_takes_the_fused_dg_maxstep_trial_with_active_bounds(A):
    """non-negative least squares: bounds active at the start and at the end; every iteration's first trial is handed out by
    the dg / max-step pass"""
    core, _ = A.load()
    R_, n, iters = 300, 40, 15
    rng, m, dense = _regression(R_, n, 79, per_row=5)
    b = dense @ rng.standard_normal(n)
    f = A.LinearObjective(LR.SQUARE, m, n, data=(b,))
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
    assert abs(fx - 0.5 * float(r @ r)) <= 1e-10 * max(1.0, fx)


# ---------------------------------------------------------------- refusals
def _nothing_bound(c):
    fx, g2, x2 = _d(3)
    before = _launches(c.core)
    assert c.core.lbfgsx_eval(c.h, c.L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
    assert _launches(c.core) == before
    assert c.core.lbfgsx_objective_linear_topology(c.h, None, None, None, None, None, None, None) == c.L.E_INVALID


def test_offending_matrices_are_refused_by_value_and_nothing_is_evaluated(A):
    n = 6
    good = ([0, 2, 2, 5], [0, 3, 5, 1, 4], [1.0, 2.0, 3.0, 4.0, 5.0])  # R = 3, nnz = 5
    with Ctx(A, O.F64, n) as c:
        L = c.L
        h = _compile(c, LR.HINGE)

        def bind(m, R_=None, nnz=None, handle=h, lanes=0, oid=None):
            rp, col, val = np.asarray(m[0], np.int32), np.asarray(m[1], np.int32), np.asarray(m[2], np.float64)
            return c.core.lbfgsx_objective_bind_linear(c.h, handle, len(m[0]) - 1 if R_ is None else R_,
                                                       len(m[1]) if nnz is None else nnz, _vp(rp), _vp(col), _vp(val), 0, lanes,
                                                       None, None, oid)
        cases = [("rowptr[0] != 0", ([1, 2, 2, 5], good[1], good[2]), "rowptr[0] = 1 with R = 3, nnz = 5", 1),
                 ("rowptr decreases", ([0, 3, 2, 5], good[1], good[2]), "rowptr[2] = 2 with R = 3, nnz = 5", 1),
                 ("rowptr[R] != nnz", ([0, 2, 2, 4], good[1], good[2]), "rowptr[3] = 4 with R = 3, nnz = 5", 1),
                 ("rowptr[R] > nnz", ([0, 2, 2, 9], good[1], good[2]), "rowptr[3] = 9 with R = 3, nnz = 5", 1),
                 ("col = -1", (good[0], [0, 3, -1, 1, 4], good[2]), "col[2] = -1 with n = 6", 1),
                 ("col = n", (good[0], [0, 3, 5, 6, 4], good[2]), "col[3] = 6 with n = 6", 1),
                 ("two offenders", (good[0], [0, 7, 5, 1, 9], good[2]), "col[1] = 7 with n = 6", 2),
                 ("rowptr before col", ([0, 3, 2, 5], [0, 7, 5, 1, 9], good[2]), "rowptr[2] = 2 with R = 3, nnz = 5", 3)]
        for name, m, what, count in cases:
            assert bind(good) == 0  # something is bound before each refusal
            before = _launches(c.core)
            rc = bind(m, oid=C.byref(C.c_int(-1)))
            assert rc == L.E_INVALID and what in L.last_error(), L.last_error()
            assert "%d of the 9 positions" % count in L.last_error(), L.last_error()
            assert _launches(c.core) == before + 1, name + ": only the validation kernel runs on unchecked indices"
            _nothing_bound(c)
        lim = 2 ** 31
        for kw, what in ((dict(R_=0), "R = 0, nnz = 5"), (dict(R_=-2), "R = -2, nnz = 5"), (dict(nnz=0), "R = 3, nnz = 0"),
                         (dict(R_=lim), "R = 2147483648 exceeds 2^31 - 1"), (dict(nnz=lim), "nnz = 2147483648 exceeds 2^31 - 1"),
                         (dict(lanes=3), "lanes = 3"), (dict(lanes=128), "lanes = 128"), (dict(lanes=-1), "lanes = -1")):
            assert bind(good) == 0
            before = _launches(c.core)
            assert bind(good, **kw) == L.E_INVALID and what in L.last_error(), L.last_error()
            assert _launches(c.core) == before
            _nothing_bound(c)
        assert bind(good) == 0
        fc = A.ChainObjective("g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];", K=2)
        assert bind(good, handle=fc.compile()) == L.E_INVALID
        assert "the handle is a chain objective, not a linear-model objective" in L.last_error()
        _nothing_bound(c)
        assert bind(good) == 0
        f32 = A.LinearObjective(LR.HINGE, good, n)
        assert bind(good, handle=f32.compile(np.float32)) == L.E_INVALID and "the other dtype" in L.last_error()
        _nothing_bound(c)
        # the other bind calls refuse a linear-model handle
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID
        assert "a linear-model objective is bound with its matrix: lbfgsx_objective_bind_linear" in L.last_error()
        i32p = C.POINTER(C.c_int32)
        e0 = np.zeros(5, np.int32).ctypes.data_as(i32p)
        assert c.core.lbfgsx_objective_bind_graph(c.h, h, 5, e0, e0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a linear-model objective, not a graph objective" in L.last_error()
        assert c.core.lbfgsx_objective_bind_mesh(c.h, h, 1, e0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a linear-model objective, not a mesh objective" in L.last_error()
        assert c.core.lbfgsx_objective_bind_grid(c.h, h, 2, 3, None, None, None) == L.E_INVALID
        assert "the handle is a linear-model objective, not a grid objective" in L.last_error()
        # and a good matrix binds, every lane count
        for lanes in (0, 1, 2, 4, 8, 16, 32, 64):
            oid = C.c_int(-1)
            assert bind(good, lanes=lanes, oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
            assert _info(c)["L"] == (lanes or 1)
    # through the solver: ValueError with the position named
    for m, what in ((([0, 1, 2], [0, 6], [1.0, 1.0]), "col\\[1\\] = 6 with n = 6"),
                    (([0, 2, 1, 2], [0, 1], [1.0, 1.0]), "rowptr\\[2\\] = 1 with R = 3, nnz = 2")):
        with pytest.raises(ValueError, match=what):
            A.LBFGSSolver(A.LBFGSParam()).minimize(A.LinearObjective(LR.HINGE, m, 6, data=(np.ones(len(m[0]) - 1),)), np.zeros(6))


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    P = LR.random_rows(50, 64, 6, 3, np.float64)
    f = A.LinearObjective(LR.HINGE, (P.rowptr, P.col, P.val), 64, coord_body=LR.RIDGE, data=(P.p0,), scalars=(0.1,))
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
