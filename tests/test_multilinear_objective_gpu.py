"""-m gpu: multi-output linear-model objectives (lbfgspp_amd.MultiLinearObjective, csrc/linear_multi_kernels.cuh,
csrc/linear_topology.hip) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders, a stale trial vector in
    place), lbfgsx_b_eval and lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/multilinear_ref.py -- gradient
    and written x bit for bit, f and the dot products adjacent to the exact sums (tests/statement_ref.py), extrema exactly
    equal -- for two row bodies with and without a ridge, at the smallest shapes at which each path can go wrong
    (multilinear_ref.problem).  Launches are counted (6 per bind, 2 per evaluation, 3 with a long column) and the model bytes
    follow the formulas;
  * at D = 1 the form gives the scalar form's bits; lbfgsx_objective_linear_topology is the transposed list of the R x F
    matrix with info[6] = D; device-resident CSR arrays and the Python class with both array kinds;
  * the multi-class hinge with a ridge and multi-target non-negative least squares follow the reference
    (tests/golden/multilinear_golden.json), from Python and C++;
  * softmax regression converges under both solvers; L-BFGS-B takes the fused dg / max-step trial; refusals by value."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import linear_ref as LR
import multilinear_ref as MR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_multilinear_objective_cpu import SOFTMAX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
BIND_LAUNCHES = 6            # validation, expansion, sort, column offsets, entries, long-column search
BODIES = [("coupled", False), ("coupled", True), ("mhinge", False), ("mhinge", True)]
NAMES = ("single", "tiny", "random", "wide16", "tile", "long")
LANES = {"single": (0, 2), "tiny": (0, 4), "random": (0, 1, 2, 8, 64), "wide16": (0,), "tile": (0,), "long": (0,)}
CASES = [pytest.param(dt, name, id="%s-%s" % ("f64" if dt == O.F64 else "f32", name)) for dt in (O.F64, O.F32) for name in NAMES]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


_compiled, _problems = {}, {}


def _problem(name, dtype):
    """computed once and shared: a Problem caches the row sums of every x it has seen"""
    if (name, dtype) not in _problems:
        _problems[(name, dtype)] = MR.problem(name, NPDT[dtype])
    return _problems[(name, dtype)]


def _compile(c, D, row, coord=None):
    key = (D, row, coord, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_linear_multi(C.byref(h), c.dtype, D, coord.encode() if coord else None, row.encode(),
                                                          log, len(log))
        assert rc == 0 and h.value, log.value.decode()
        info = (C.c_longlong * 8)()
        assert c.core.lbfgsx_objective_info(h, C.byref(info)) == 0 and info[1] == 0  # zero scratch, all six kernels
        _compiled[key] = h
    return _compiled[key]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _info(c):
    info = (C.c_int64 * 8)()
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, C.byref(info), None, None, None, None, None, None))
    return dict(zip(("R", "nnz", "L", "C", "nlong", "nchunks", "D"), list(info)[:7]))


def _model_bytes(core):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), 0) == 0
    return cnt[3]


def _lin_bytes(M, esz, vg, nchunks):
    """the byte model of one evaluation (launch_args.hpp): the offsets of both passes (R + 1 and F + 1 words), their indices
    and matrix values once; D times the gathered values (vg vectors in the row pass, w in the column pass), w written and
    read and the chunk partials written and read; v written and read"""
    return ((M.R + 1) * 4 + (M.F + 1) * 4 + 2 * M.nnz * 4 + 2 * M.nnz * esz + M.nnz * esz * (vg + 1) * M.D + 2 * M.R * esz * M.D
            + 2 * M.R * esz + 2 * nchunks * esz * M.D)


def _bind(c, M, row, with_ridge, lanes):
    """compiles (once per process) and binds the row body (and RIDGE) with M's data; returns (id, chunks, x -> (g, terms))"""
    L = c.L
    dev = C.c_void_p()
    p0 = M.p0(row)
    L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, _vp(p0), p0.size, C.byref(dev)))
    ptrs = (C.c_void_p * 4)()
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(M.c0, M.c1, *([0.0] * 6))
    oid = C.c_int(-1)
    rp, col, val = M.rowptr.copy(), M.col.copy(), M.val.copy()
    h = _compile(c, M.D, MR.ROW_BODIES[row][0], MR.RIDGE if with_ridge else None)
    before = _launches(c.core)
    L.check(c.core.lbfgsx_objective_bind_linear(c.h, h, M.R, M.nnz, _vp(rp), _vp(col), _vp(val), 0, lanes, C.byref(ptrs),
                                                C.byref(cs), C.byref(oid)))
    assert _launches(c.core) == before + BIND_LAUNCHES
    rp[:] = -5  # the binding keeps its own copies
    col[:] = -5
    val[:] = 0
    assert oid.value == L.OBJ_BOUND
    lanes_used = lanes or LR.lanes_rule(M.R, M.nnz)
    info = _info(c)
    assert (info["R"], info["nnz"], info["L"], info["C"], info["D"]) == (M.R, M.nnz, lanes_used, MR.C_DEFAULT, M.D)
    assert (info["nlong"] > 0) == M.has_long()
    assert info["nchunks"] == LR.chunk_table(M.topo[0])[2].shape[0]
    return oid.value, info["nchunks"], lambda x: M.evaluate(x, lanes_used, row, with_ridge)


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,name", CASES)
def test_eval_and_trial_statements_in_both_tile_orders(A, dtype, name):
    M = _problem(name, dtype)
    n = M.n
    per_eval = 3 if M.has_long() else 2
    rng = np.random.default_rng(100 + n)
    with Ctx(A, dtype, n) as c:
        L, dt = c.L, c.dt
        esz = np.dtype(dt).itemsize
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
                oid, nchunks, ref = _bind(c, M, row, with_ridge, lanes)
                fx, g2, x2 = _d(3)
                before, bytes0 = _launches(c.core), _model_bytes(c.core)
                L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
                assert _launches(c.core) == before + per_eval
                assert _model_bytes(c.core) - bytes0 == _lin_bytes(M, esz, 1, nchunks), what
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
                    before, bytes0 = _launches(c.core), _model_bytes(c.core)
                    L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                    assert _launches(c.core) == before + per_eval
                    # a trial launch reads xp and d, writes x and grad and reads the one data array
                    assert _model_bytes(c.core) - bytes0 == n * esz * (4 + 1) + _lin_bytes(M, esz, 2, nchunks), what
                    _bits(c.down(L.VEC_XT), xt_ref, "%s launch %d: x trial" % (what, k))
                    _bits(c.down(L.VEC_GT), g_ref, "%s launch %d: g trial" % (what, k))
                    runs.append((fx.value, dg.value))
                assert runs[0] == runs[1], what + ": f or g.d depends on the tile order"
                _sum_ok(runs[0][0], terms, dt, what + ": f trial")
                _dot_ok(runs[0][1], g_ref, d, dt, what + ": g.d")
                assert M.nnz < 100 or np.any(g_ref != 0)
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,name", CASES)
def test_b_eval_and_dg_maxstep_trial_statements(A, monkeypatch, dtype, name):
    """lbfgsx_b_eval, then the fused first trial of L-BFGS-B with some bounds active: g.d and step_max, and the trial point, its
    gradient, f and grad.d that lbfgsx_trial then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    M = _problem(name, dtype)
    n = M.n
    per_eval = 3 if M.has_long() else 2
    rng = np.random.default_rng(300 + n)
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        esz = np.dtype(dt).itemsize
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for lanes in LANES[name]:
            for row, with_ridge in BODIES:
                what = "%s lanes %d %s%s" % (name, lanes, row, "+ridge" if with_ridge else "")
                oid, nchunks, ref = _bind(c, M, row, with_ridge, lanes)
                for which, arr in ((L.VEC_X, x), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                    c.up(which, arr)
                fx, pg, x2 = _d(3)
                before, bytes0 = _launches(c.core), _model_bytes(c.core)
                L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
                assert _launches(c.core) == before + per_eval
                assert _model_bytes(c.core) - bytes0 == _lin_bytes(M, esz, 1, nchunks), what
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
                before, bytes0 = _launches(c.core), _model_bytes(c.core)
                L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
                assert _launches(c.core) == before + per_eval  # the first trial rides on the dg / max-step pass
                # xp, g, d, lb, ub read, x and grad written, the one data array read
                assert _model_bytes(c.core) - bytes0 == n * esz * (7 + 1) + _lin_bytes(M, esz, 2, nchunks), what
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


# ---------------------------------------------------------------- D = 1 is the scalar form
def _scalar_problem(name, dtype):
    return LR.random_rows(700, 1031, 40, 7, NPDT[dtype]) if name == "random" else LR.long_columns(NPDT[dtype])


@pytest.mark.parametrize("dtype", [O.F64, O.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["random", "long"])
def test_one_output_gives_the_bits_of_the_scalar_form(A, dtype, name):
    """the multi-output form compiled with z[0] / dz[0] bodies against LinearObjective's kernels on the same matrix: g, f and
    the outputs of both trial kernels bit for bit"""
    P = _scalar_problem(name, dtype)
    n = P.n
    x, d, lb, ub = R.bound_cases(np.random.default_rng(500 + n), n, NPDT[dtype])["mixed_one_sided"]
    got = {}
    for form in ("scalar", "multi"):
        with Ctx(A, dtype, n, bounded=True) as c:
            L = c.L
            dev = C.c_void_p()
            L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, _vp(P.p0), P.R, C.byref(dev)))
            ptrs = (C.c_void_p * 4)()
            ptrs[0] = dev.value
            cs = (C.c_double * 8)(P.c0, *([0.0] * 7))
            out = []
            for row in (LR.CUBIC, LR.LOGISTIC):
                h = C.c_void_p()
                log = C.create_string_buffer(8192)
                if form == "scalar":
                    rc = c.core.lbfgsx_objective_compile_linear(C.byref(h), c.dtype, LR.RIDGE.encode(), row.encode(), log, len(log))
                else:
                    rc = c.core.lbfgsx_objective_compile_linear_multi(C.byref(h), c.dtype, 1, LR.RIDGE.encode(),
                                                                      MR.scalar_body(row).encode(), log, len(log))
                assert rc == 0, log.value.decode()
                oid = C.c_int(-1)
                L.check(c.core.lbfgsx_objective_bind_linear(c.h, h, P.R, P.nnz, _vp(P.rowptr), _vp(P.col), _vp(P.val), 0, 0,
                                                            C.byref(ptrs), C.byref(cs), C.byref(oid)))
                assert _info(c)["D"] == (0 if form == "scalar" else 1)
                for which, arr in ((L.VEC_X, x), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                    c.up(which, arr)
                r3, r2, b3, b2, t2 = _d(3), _d(2), _d(3), _d(2), _d(2)
                L.check(c.core.lbfgsx_eval(c.h, oid.value, *[C.byref(v) for v in r3]))
                out.append(c.down(L.VEC_G).copy())
                L.check(c.core.lbfgsx_ls_begin(c.h))
                L.check(c.core.lbfgsx_trial(c.h, oid.value, 0.37, *[C.byref(v) for v in r2]))
                out += [c.down(L.VEC_XT).copy(), c.down(L.VEC_GT).copy()]
                c.up(L.VEC_X, x)
                L.check(c.core.lbfgsx_b_eval(c.h, oid.value, *[C.byref(v) for v in b3]))
                out.append(c.down(L.VEC_G).copy())
                L.check(c.core.lbfgsx_ls_begin(c.h))
                L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid.value, 0.21, *[C.byref(v) for v in b2]))
                out += [c.down(L.VEC_XT).copy(), c.down(L.VEC_GT).copy()]
                L.check(c.core.lbfgsx_trial(c.h, oid.value, 0.21, *[C.byref(v) for v in t2]))
                out.append(np.array([v.value for v in r3 + r2 + b3 + b2 + t2]))
                c.core.lbfgsx_objective_destroy(h)
            got[form] = out
    assert len(got["scalar"]) == len(got["multi"]) == 14
    for k, (a, b) in enumerate(zip(got["scalar"], got["multi"])):
        _bits(b, a, "%s output %d" % (name, k))
        assert np.any(a != 0)


# ---------------------------------------------------------------- the topology
def _read_topology(c, M):
    info = _info(c)
    colptr, trow, tpos = np.full(M.F + 1, 7, np.uint32), np.full(M.nnz, 7, np.int32), np.full(M.nnz, 7, np.uint32)
    long_col, long_chunk = np.full(info["nlong"], 7, np.int32), np.full(info["nlong"] + 1, 7, np.uint32)
    chunk = np.full((info["nchunks"], 2), 7, np.uint32)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    c.L.check(c.core.lbfgsx_objective_linear_topology(c.h, None, colptr.ctypes.data_as(u32p), trow.ctypes.data_as(i32p),
                                                      tpos.ctypes.data_as(u32p), long_col.ctypes.data_as(i32p),
                                                      long_chunk.ctypes.data_as(u32p), chunk.ctypes.data_as(u32p)))
    return info, (colptr, trow, tpos), (long_col, long_chunk, chunk)


def _topology_matches(c, M, lanes):
    info, topo, table = _read_topology(c, M)
    assert info["L"] == (lanes or LR.lanes_rule(M.R, M.nnz)) and info["D"] == M.D
    for got, want in zip(topo, M.topo):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    want = LR.chunk_table(M.topo[0])
    if info["nlong"] == 0:
        assert want[0].size == 0 and info["nchunks"] == 0
    else:
        for got, w in zip(table, want):
            assert got.dtype == w.dtype and np.array_equal(got, w)


@pytest.mark.parametrize("name", ["single", "tiny", "random", "wide16", "long"])
def test_topology_is_the_transposed_list_of_the_R_by_F_matrix(A, name):
    M = _problem(name, O.F64)
    with Ctx(A, O.F64, M.n) as c:
        for lanes in LANES[name]:
            _bind(c, M, "mhinge", False, lanes)
            _topology_matches(c, M, lanes)


def test_matrix_arrays_may_be_device_arrays(A):
    """matrix_on_device = 1: the same list and the same gradient bits from device copies of the three arrays (here: three of
    the context's own data buffers, which hold the int32 words as raw bytes)"""
    M = MR.Problem(LR.random_rows(200, 64, 9, 21, np.float32), 5, 11)  # f32: an element of a data buffer is 4 bytes, as an index
    with Ctx(A, O.F32, M.n) as c:
        L = c.L
        x = np.random.default_rng(5).standard_normal(M.n).astype(np.float32)
        c.up(L.VEC_X, x)
        oid, _, ref = _bind(c, M, "mhinge", True, 0)
        fx, g2, x2 = _d(3)
        L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
        want = (c.down(L.VEC_G).copy(), fx.value)
        dev = [C.c_void_p() for _ in range(4)]
        for slot, arr in ((0, M.labels), (1, M.rowptr), (2, M.col), (3, M.val)):
            L.check(c.core.lbfgsx_objective_upload_count(c.h, slot, _vp(arr), arr.size, C.byref(dev[slot])))
        ptrs = (C.c_void_p * 4)()
        ptrs[0] = dev[0].value
        cs = (C.c_double * 8)(M.c0, M.c1, *([0.0] * 6))
        oid = C.c_int(-1)
        L.check(c.core.lbfgsx_objective_bind_linear(c.h, _compile(c, M.D, MR.MHINGE, MR.RIDGE), M.R, M.nnz, dev[1], dev[2], dev[3],
                                                    1, 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
        _topology_matches(c, M, 0)
        L.check(c.core.lbfgsx_eval(c.h, oid.value, C.byref(fx), C.byref(g2), C.byref(x2)))
        _bits(c.down(L.VEC_G), want[0], "g from the device arrays")
        _bits(want[0], ref(x)[0], "g against the restatement")
        assert fx.value == want[1]


def test_python_class_takes_numpy_arrays_and_device_tensors(A):
    """MultiLinearObjective with the matrix as numpy arrays and as torch tensors on the device: the same iterates, bit for bit"""
    import torch
    M = MR.Problem(LR.random_rows(300, 40, 12, 33, np.float64), 3, 12)
    lam = 0.1
    x0 = np.random.default_rng(6).standard_normal(M.n)
    out = []
    for dev in (False, True):
        m = (M.rowptr, M.col, M.val)
        if dev:
            m = tuple(torch.from_numpy(a.copy()).cuda() for a in m)
        f = A.MultiLinearObjective(MR.MHINGE, m, M.F, M.D, coord_body=MR.RIDGE, data=(M.labels,), scalars=(lam,))
        assert f.on_device == dev and f.n == M.n
        s = A.LBFGSSolver(A.LBFGSParam(m=5, epsilon=0, epsilon_rel=0, max_iterations=8), linesearch=A.LS_MORE_THUENTE)
        x = x0.copy()
        niter, fx = s.minimize(f, x)
        out.append((niter, s.last.nfev, fx, x))
    assert out[0][:3] == out[1][:3] and out[0][0] == 8
    _bits(out[1][3], out[0][3], "x from device tensors")
    Z = MR.row_sums(M.rowptr, M.col, M.val, x0.reshape(M.F, M.D), LR.lanes_rule(M.R, M.nnz))
    f0 = float(np.sum(MR.mhinge(Z, M.labels)[1]) + np.sum(LR.ridge(x0, lam)[1]))
    assert out[0][2] < f0  # it went down from the start value
    with pytest.raises(ValueError, match="n = 121 is not a multiple of D = 3"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f, np.zeros(121))


# ---------------------------------------------------------------- against the reference
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "multilinear_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10
    return g


SQUARES = """
T q = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    const T u = z[k] - p0[r * D + k];
    dz[k] = u;
    q = q + u * u;
}
return T(0.5) * q;"""


def _probe_instance(A, solver, R_, F, D, k):
    """tests/cpp/multilinear_probe.cpp: the matrix, the per-row data and start(), operation for operation"""
    r, j = np.arange(R_)[:, None], np.arange(k["per"])[None, :]
    col = ((7 * r + 3 * j * j + j) % F).reshape(-1)
    val = (((31 * r + 17 * j) % 13 - 6) / 4.0).reshape(-1)
    rowptr = np.arange(0, R_ * k["per"] + 1, k["per"])
    y = ((5 * r) % D).reshape(-1).astype(np.float64)
    b = (((11 * r + 5 * np.arange(D)[None, :]) % 7 - 3) / 2.0).reshape(-1)
    n = F * D
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    x0 = k["amp"] * ((0.5 - t) * (1.0 + t))
    if solver == "lbfgs":
        return A.MultiLinearObjective(MR.MHINGE, (rowptr, col, val), F, D, coord_body=MR.RIDGE, data=(y,), scalars=(k["c0"],)), x0
    return A.MultiLinearObjective(SQUARES, (rowptr, col, val), F, D, data=(b,)), x0


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%dx%dx%d" % (i["solver"], i["R"], i["F"], i["D"]))
def test_multi_output_models_follow_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
    assert inst["iterations"] >= 8 and n == inst["F"] * inst["D"]
    f, x0 = _probe_instance(A, inst["solver"], inst["R"], inst["F"], inst["D"], _golden()["constants"])
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


def test_cpp_multi_linear_objective_follows_the_reference(tmp_path):
    """tests/cpp/multilinear_probe.cpp with MultiLinearObjective<double> in place of the functor, built with g++ against
    include/"""
    exe = str(tmp_path / "multilinear_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DMULTILINEAR_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "multilinear_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["R"], i["F"], i["D"]) for i in insts}):
        mine = [i for i in insts if (i["R"], i["F"], i["D"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe] + [str(v) for v in shape] + [str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert out.returncode == 0 and "MULTILINEAR PROBE OK" in out.stdout, out.stdout[-2000:]
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
def test_softmax_regression_converges(A, solver):
    """f = (1/R) sum_r (logsumexp(Z[r, :]) - Z[r, y_r]) + lam/2 |x|^2, 400 x 21 (20 features and an intercept column of ones),
    D = 4.  At the returned x the dense float64 numpy gradient (logsumexp) meets the solver's own stopping rule with a factor
    2: ||g|| <= 2 eps max(1, ||x||).  The device and numpy gradients differ only by the rounding of exp (400 terms of size
    <= 1/R each: about 1e-15), orders of magnitude below eps = 1e-6, so the factor cannot hide a wrong gradient.  eps = 1e-6 as
    in the scalar form's tests: at 1e-8 the decrease falls under the spacing of f"""
    R_, F, D, eps, lam = 400, 21, 4, 1e-6, 1e-2
    rng = np.random.default_rng(81)
    dense = rng.standard_normal((R_, F))
    dense[:, 0] = 1.0
    dense[rng.random((R_, F)) < 0.5] = 0.0
    dense[:, 0] = 1.0
    rows, cols = np.nonzero(dense)
    m = (np.concatenate([[0], np.cumsum(np.count_nonzero(dense, axis=1))]), cols, dense[rows, cols])
    y = np.argmax(dense @ rng.standard_normal((F, D)) + 0.5 * rng.standard_normal((R_, D)), axis=1)
    assert "#pragma unroll" in SOFTMAX
    f = A.MultiLinearObjective(SOFTMAX, m, F, D, coord_body=MR.RIDGE, data=(y.astype(np.float64),), scalars=(lam, 1.0 / R_))
    n, cap = F * D, 3000
    x = np.zeros(n)
    if solver == "lbfgs":
        s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap), linesearch=A.LS_MORE_THUENTE)
        niter, fx = s.minimize(f, x)
    else:
        s = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=eps, epsilon_rel=eps, past=0, max_iterations=cap))
        niter, fx = s.minimize(f, x, np.full(n, -50.0), np.full(n, 50.0))
        assert np.abs(x).max() < 50.0  # no bound is active: the projected gradient is the gradient
    assert 0 < niter < cap  # the solver reports convergence: it stopped by its own rule
    X = x.reshape(F, D)
    Z = dense @ X
    lse = np.logaddexp.reduce(Z, axis=1)
    P = np.exp(Z - lse[:, None])
    P[np.arange(R_), y] -= 1.0
    g = (dense.T @ P / R_ + lam * X).reshape(-1)
    f_np = float(np.mean(lse - Z[np.arange(R_), y]) + 0.5 * lam * (x @ x))
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    measure = float(np.linalg.norm(g)) if solver == "lbfgs" else float(np.abs(g).max())
    print("%s: niter %d nfev %d fx %.12g (numpy %.12g) stopping measure %.3g (bound %.3g)" % (solver, niter, s.last.nfev, fx, f_np,
                                                                                                measure, bound))
    assert measure <= 2.0 * bound
    assert abs(fx - f_np) <= 1e-11 * max(1.0, abs(f_np))
    assert np.any(X[0] != 0)  # the intercepts moved


def test_lbfgsb_solve_takes_the_fused_dg_maxstep_trial_with_active_bounds(A):
    """multi-target non-negative least squares: bounds active at the start and at the end; every iteration's first trial is
    handed out by the dg / max-step pass"""
    core, _ = A.load()
    R_, F, D, iters = 300, 20, 3, 15
    P = LR.random_rows(R_, F, 8, 79, np.float64)
    rng = np.random.default_rng(80)
    dense = np.zeros((R_, F))
    np.add.at(dense, (np.repeat(np.arange(R_), np.diff(P.rowptr)), P.col), P.val)
    B = dense @ rng.standard_normal((F, D))
    f = A.MultiLinearObjective(SQUARES, (P.rowptr, P.col, P.val), F, D, data=(B.reshape(-1),))
    n = F * D
    s = A.LBFGSBSolver(A.LBFGSBParam(m=6, epsilon=0, epsilon_rel=0, past=0, max_iterations=iters))
    s.prepare(n)
    lb, ub = np.zeros(n), np.full(n, np.inf)
    x = np.zeros(n)
    f0 = 0.5 * float((B * B).sum())
    niter, fx = s.minimize(f, x, lb, ub)
    ahead = (C.c_int64 * 2)()
    assert core.lbfgsx_b_trial_ahead_counts(s.ctx, C.byref(ahead)) == 0
    print(niter, s.last.nfev, fx, f0, ahead[0], ahead[1])
    assert niter > 0 and ahead[0] > 0 and ahead[1] > 0  # lbfgsx_b_dg_maxstep_trial ran, and its trial was taken over
    assert fx < f0 and (x >= 0).all() and (x == 0).any() and (x > 0).any()
    r = dense @ x.reshape(F, D) - B
    assert abs(fx - 0.5 * float((r * r).sum())) <= 1e-10 * max(1.0, fx)


# ---------------------------------------------------------------- refusals
def _nothing_bound(c):
    fx, g2, x2 = _d(3)
    before = _launches(c.core)
    assert c.core.lbfgsx_eval(c.h, c.L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
    assert _launches(c.core) == before
    assert c.core.lbfgsx_objective_linear_topology(c.h, None, None, None, None, None, None, None) == c.L.E_INVALID


def test_offending_requests_are_refused_by_value_and_nothing_is_evaluated(A):
    n, D = 6, 3  # F = 2
    good = ([0, 2, 2, 5], [0, 1, 1, 1, 0], [1.0, 2.0, 3.0, 4.0, 5.0])  # R = 3, nnz = 5
    name = "multi-output linear-model objective"
    with Ctx(A, O.F64, n) as c:
        L = c.L
        h = _compile(c, D, MR.MHINGE)
        h_scalar = C.c_void_p()
        log = C.create_string_buffer(4096)
        assert c.core.lbfgsx_objective_compile_linear(C.byref(h_scalar), c.dtype, None, LR.HINGE.encode(), log, len(log)) == 0

        def bind(m, handle=h, oid=None):
            rp, col, val = np.asarray(m[0], np.int32), np.asarray(m[1], np.int32), np.asarray(m[2], np.float64)
            return c.core.lbfgsx_objective_bind_linear(c.h, handle, len(m[0]) - 1, len(m[1]), _vp(rp), _vp(col), _vp(val), 0, 0,
                                                       None, None, oid)
        # col = 2 and col = 5 lie in [0, n) but not in [0, F): the scalar handle takes them, the multi-output one does not
        for m, what, count in (((good[0], [0, 1, 2, 1, 0], good[2]), "col[2] = 2 with F = n / D = 6 / 3 = 2", 1),
                               ((good[0], [0, 5, 1, 1, 2], good[2]), "col[1] = 5 with F = n / D = 6 / 3 = 2", 2),
                               ((good[0], [0, -1, 1, 1, 0], good[2]), "col[1] = -1 with F = n / D = 6 / 3 = 2", 1)):
            assert bind(good) == 0  # something is bound before each refusal
            before = _launches(c.core)
            rc = bind(m, oid=C.byref(C.c_int(-1)))
            assert rc == L.E_INVALID and name + ": " + what in L.last_error(), L.last_error()
            assert "%d of the 9 positions" % count in L.last_error(), L.last_error()
            assert _launches(c.core) == before + 1, "only the validation kernel runs on unchecked indices"
            _nothing_bound(c)
            if min(m[1]) >= 0:
                assert bind(m, handle=h_scalar) == 0  # valid against n
        # a scalar-linear handle still binds, and reports D = 0
        oid = C.c_int(-1)
        assert bind(good, handle=h_scalar, oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND and _info(c)["D"] == 0
        assert bind(good, oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND and _info(c)["D"] == D
        # the other bind calls refuse a multi-output handle
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID
        assert "a %s is bound with its matrix: lbfgsx_objective_bind_linear" % name in L.last_error()
        assert "bind_linear_multi" not in L.last_error()
        i32p = C.POINTER(C.c_int32)
        e0 = np.zeros(5, np.int32).ctypes.data_as(i32p)
        assert c.core.lbfgsx_objective_bind_graph(c.h, h, 5, e0, e0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a %s, not a graph objective" % name in L.last_error()
        _nothing_bound(c)
        assert c.core.lbfgsx_objective_bind_mesh(c.h, h, 1, e0, 0, None, None, None) == L.E_INVALID
        assert "the handle is a %s, not a mesh objective" % name in L.last_error()
        _nothing_bound(c)
        assert c.core.lbfgsx_objective_bind_grid(c.h, h, 2, 3, None, None, None) == L.E_INVALID
        assert "the handle is a %s, not a grid objective" % name in L.last_error()
        c.core.lbfgsx_objective_destroy(h_scalar)
    # n % D != 0: both values named, no launch
    with Ctx(A, O.F64, 7) as c:
        L = c.L
        h = _compile(c, D, MR.MHINGE)
        rp, col, val = np.asarray(good[0], np.int32), np.asarray(good[1], np.int32), np.asarray(good[2], np.float64)
        before = _launches(c.core)
        rc = c.core.lbfgsx_objective_bind_linear(c.h, h, 3, 5, _vp(rp), _vp(col), _vp(val), 0, 0, None, None, None)
        assert rc == L.E_INVALID and name + ": n = 7 is not a multiple of D = 3" in L.last_error(), L.last_error()
        assert _launches(c.core) == before
        _nothing_bound(c)
    # through the solver: ValueError with the position named
    with pytest.raises(ValueError, match="col\\[1\\] = 2 with F = n / D = 6 / 3 = 2"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(
            A.MultiLinearObjective(MR.MHINGE, ([0, 1, 2], [0, 2], [1.0, 1.0]), 2, 3, data=(np.zeros(2),)), np.zeros(6))


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    M = MR.Problem(LR.random_rows(50, 16, 6, 3, np.float64), 4, 13)
    f = A.MultiLinearObjective(MR.MHINGE, (M.rowptr, M.col, M.val), M.F, M.D, coord_body=MR.RIDGE, data=(M.labels,), scalars=(0.1,))
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
