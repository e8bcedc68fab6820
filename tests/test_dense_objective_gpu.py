"""-m gpu: dense linear-model objectives (lbfgspp_amd.DenseLinearObjective, csrc/linear_dense_kernels.cuh,
csrc/dense_topology.hip) on the device.

  * statement level: one evaluation through each of lbfgsx_eval, lbfgsx_trial (twice: both tile orders, a stale trial vector in
    place), lbfgsx_b_eval and lbfgsx_b_dg_maxstep_trial against the numpy restatement of tests/dense_ref.py -- gradient, written
    x, w, v and the chunk partials bit for bit, f and the dot products adjacent to the exact sums (tests/statement_ref.py),
    extrema exactly equal -- for coupled least squares and the squared hinge with and without a ridge, at the smallest shapes
    at which each pass can go wrong (dense_ref.SHAPES); softmax, whose exp and log numpy does not round as the device does,
    has its partials and gradient bit for bit from the device's own w, and w and v against numpy to a few ulps.  Launches are
    counted (3 per evaluation, none per bind) and the model bytes follow the formula of include/lbfgsx.h;
  * the same matrix as full CSR through the sparse forms gives the same bits in w, v and f and a gradient within the bound of
    two summation orders;
  * every instance of the sparse forms' reference fixtures, its matrix densified, follows the reference;
  * softmax regression converges under both solvers; a device matrix is used in place; L-BFGS-B takes the fused dg / max-step
    trial at every iteration; refusals by value."""
import base64
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import dense_ref as DR
import linear_ref as LR
import multilinear_ref as MR
import oracle_lib as O
import statement_ref as R
from test_driver_statements_gpu import Ctx, _ahead, _bits, _d, _dot_ok, _launches, _sum_ok
from test_multilinear_objective_cpu import SOFTMAX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {O.F64: np.float64, O.F32: np.float32}
BODIES = [("coupled", False), ("coupled", True), ("mhinge", False), ("mhinge", True)]
NAMES = tuple(DR.SHAPES)
LANES = {name: (0,) for name in NAMES}
LANES["f65"] = (0, 1, 8, 64)
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
        _problems[(name, dtype)] = DR.problem(name, NPDT[dtype])
    return _problems[(name, dtype)]


def _compile(c, D, row, coord=None):
    key = (D, row, coord, c.dtype)
    if key not in _compiled:
        h = C.c_void_p()
        log = C.create_string_buffer(8192)
        rc = c.core.lbfgsx_objective_compile_dense(C.byref(h), c.dtype, D, coord.encode() if coord else None, row.encode(), log,
                                                   len(log))
        assert rc == 0 and h.value, log.value.decode()
        info = (C.c_longlong * 8)()
        assert c.core.lbfgsx_objective_info(h, C.byref(info)) == 0 and info[1] == 0  # zero scratch, all seven kernels
        _compiled[key] = h
    return _compiled[key]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _info(c):
    info = (C.c_int64 * 8)()
    c.L.check(c.core.lbfgsx_objective_dense_info(c.h, C.byref(info)))
    return dict(zip(("R", "F", "D", "L", "C", "chunks", "lda", "own"), list(info)))


def _read(c, P):
    w, v, part = np.full((P.R, P.D), 7, c.dt), np.full(P.R, 7, c.dt), np.full((P.chunks, P.F, P.D), 7, c.dt)
    c.L.check(c.core.lbfgsx_objective_dense_read(c.h, _vp(w), _vp(v), _vp(part)))
    return w, v, part


def _model_bytes(core):
    cnt = (C.c_int64 * 8)()
    assert core.lbfgsx_counters_ex(C.byref(cnt), 0) == 0
    return cnt[3]


def _dense_bytes(P, s, vg):
    """the byte model of one evaluation (include/lbfgsx.h): A twice, the weights of the row pass (vg vectors), w and v written
    and read, the chunk partials written and read"""
    return 2 * P.R * P.F * s + P.n * s * vg + 2 * P.R * P.D * s + 2 * P.R * s + 2 * P.chunks * P.n * s


def _bind(c, P, row_text, p0, coord, lanes, keep):
    """compiles (once per process) and binds; a padded matrix (lda > F) goes as a device tensor, used in place.  Returns id"""
    L = c.L
    dev = C.c_void_p()
    L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, _vp(p0), p0.size, C.byref(dev)))
    ptrs = (C.c_void_p * 4)()
    ptrs[0] = dev.value
    cs = (C.c_double * 8)(P.c0, P.c1, *([0.0] * 6))
    oid = C.c_int(-1)
    h = _compile(c, P.D, row_text, coord)
    on_device = P.lda != P.F
    if on_device:
        import torch
        t = torch.from_numpy(P.Astore).cuda()
        torch.cuda.synchronize()
        keep.append(t)
        aptr = C.c_void_p(t.data_ptr())
    else:
        host = np.ascontiguousarray(P.A).copy()
        aptr = _vp(host)
    before = _launches(c.core)
    L.check(c.core.lbfgsx_objective_bind_dense(c.h, h, P.R, aptr, P.lda, 1 if on_device else 0, lanes, C.byref(ptrs), C.byref(cs),
                                               C.byref(oid)))
    assert _launches(c.core) == before  # per bind: the upload only
    if not on_device:
        host[:] = -5  # the binding keeps its own copy of a host matrix
    assert oid.value == L.OBJ_BOUND
    info = _info(c)
    want = dict(R=P.R, F=P.F, D=P.D, L=lanes or DR.lanes_rule(P.F), C=DR.C_DEFAULT, chunks=P.chunks, lda=P.lda,
                own=0 if on_device else 1)
    assert info == want, (info, want)
    return oid.value, info["L"]


def _check_passes(c, P, ref, what):
    """w, v and the chunk partials of the last evaluation against the restatement's"""
    w, v, part = _read(c, P)
    _bits(w, ref[2], what + ": w")
    _bits(v, ref[3], what + ": v")
    _bits(part, ref[4], what + ": part")


# ---------------------------------------------------------------- statement level
@pytest.mark.parametrize("dtype,name", CASES)
def test_eval_and_trial_statements_in_both_tile_orders(A, dtype, name):
    P = _problem(name, dtype)
    n = P.n
    rng = np.random.default_rng(100 + n)
    keep = []
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
                oid, lanes_used = _bind(c, P, MR.ROW_BODIES[row][0], P.p0(row), MR.RIDGE if with_ridge else None, lanes, keep)
                fx, g2, x2 = _d(3)
                before, bytes0 = _launches(c.core), _model_bytes(c.core)
                L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
                assert _launches(c.core) == before + 3
                assert _model_bytes(c.core) - bytes0 == _dense_bytes(P, esz, 1), what
                ref = P.evaluate(xp, lanes_used, row, with_ridge)
                _bits(c.down(L.VEC_G), ref[0], what + ": g")
                _check_passes(c, P, ref, what)
                _sum_ok(fx.value, ref[1], dt, what + ": f")
                _dot_ok(g2.value, ref[0], ref[0], dt, what + ": g.g")
                _dot_ok(x2.value, xp, xp, dt, what + ": x.x")
                ref = P.evaluate(xt_ref, lanes_used, row, with_ridge)
                runs = []
                for k in range(2):
                    c.up(L.VEC_XT, stale)  # whatever a launch does not write stays visible; a gather of it would show
                    c.up(L.VEC_GT, stale)
                    fx, dg = _d(2)
                    before, bytes0 = _launches(c.core), _model_bytes(c.core)
                    L.check(c.core.lbfgsx_trial(c.h, oid, step, C.byref(fx), C.byref(dg)))
                    assert _launches(c.core) == before + 3
                    # a trial launch reads xp and d, writes x and grad and reads the one data array
                    assert _model_bytes(c.core) - bytes0 == n * esz * (4 + 1) + _dense_bytes(P, esz, 2), what
                    _bits(c.down(L.VEC_XT), xt_ref, "%s launch %d: x trial" % (what, k))
                    _bits(c.down(L.VEC_GT), ref[0], "%s launch %d: g trial" % (what, k))
                    _check_passes(c, P, ref, "%s launch %d" % (what, k))
                    runs.append((fx.value, dg.value))
                assert runs[0] == runs[1], what + ": f or g.d depends on the tile order"
                _sum_ok(runs[0][0], ref[1], dt, what + ": f trial")
                _dot_ok(runs[0][1], ref[0], d, dt, what + ": g.d")
                # (with one output the multi-class hinge has no other class: its gradient is zero)
                assert np.any(ref[0] != 0) or (P.D == 1 and row == "mhinge" and not with_ridge)
        _bits(c.down(L.VEC_XP), xp, "xp is left alone")


@pytest.mark.parametrize("dtype,name", CASES)
def test_b_eval_and_dg_maxstep_trial_statements(A, monkeypatch, dtype, name):
    """lbfgsx_b_eval, then the fused first trial of L-BFGS-B with some bounds active: g.d and step_max, and the trial point, its
    gradient, f and grad.d that lbfgsx_trial then hands out without a launch"""
    monkeypatch.delenv("LBFGSX_TRIAL_AHEAD", raising=False)
    P = _problem(name, dtype)
    n = P.n
    rng = np.random.default_rng(300 + n)
    keep = []
    with Ctx(A, dtype, n, bounded=True) as c:
        L, dt = c.L, c.dt
        esz = np.dtype(dt).itemsize
        x, d, lb, ub = R.bound_cases(rng, n, dt)["mixed_one_sided"]
        g0 = rng.standard_normal(n).astype(dt)
        step0 = 0.37
        xt_ref = R.axpy_ref(x, d, step0)
        for row, with_ridge in BODIES:
            what = "%s %s%s" % (name, row, "+ridge" if with_ridge else "")
            oid, lanes_used = _bind(c, P, MR.ROW_BODIES[row][0], P.p0(row), MR.RIDGE if with_ridge else None, 0, keep)
            for which, arr in ((L.VEC_X, x), (L.VEC_D, d), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                c.up(which, arr)
            fx, pg, x2 = _d(3)
            before, bytes0 = _launches(c.core), _model_bytes(c.core)
            L.check(c.core.lbfgsx_b_eval(c.h, oid, C.byref(fx), C.byref(pg), C.byref(x2)))
            assert _launches(c.core) == before + 3
            assert _model_bytes(c.core) - bytes0 == _dense_bytes(P, esz, 1), what
            ref = P.evaluate(x, lanes_used, row, with_ridge)
            _bits(c.down(L.VEC_G), ref[0], what + ": g")
            _check_passes(c, P, ref, what)
            _sum_ok(fx.value, ref[1], dt, what + ": f")
            _dot_ok(x2.value, x, x, dt, what + ": x.x")
            assert pg.value == R.projg_norm_ref(x, ref[0], lb, ub), what
            c.up(L.VEC_G, g0)
            L.check(c.core.lbfgsx_ls_begin(c.h))
            c.up(L.VEC_XT, np.full(n, -77.0, dt))
            runs0, hits0 = _ahead(c)
            dg, sm = _d(2)
            before, bytes0 = _launches(c.core), _model_bytes(c.core)
            L.check(c.core.lbfgsx_b_dg_maxstep_trial(c.h, oid, step0, C.byref(dg), C.byref(sm)))
            assert _launches(c.core) == before + 3  # the first trial rides on the dg / max-step pass
            # xp, g, d, lb, ub read, x and grad written, the one data array read
            assert _model_bytes(c.core) - bytes0 == n * esz * (7 + 1) + _dense_bytes(P, esz, 2), what
            assert _ahead(c) == (runs0 + 1, hits0), what + ": the fused kernel did not run"
            ref = P.evaluate(xt_ref, lanes_used, row, with_ridge)
            _bits(c.down(L.VEC_XT), xt_ref, what + ": x trial left by the fused pass")
            _bits(c.down(L.VEC_GT), ref[0], what + ": g trial left by the fused pass")
            _check_passes(c, P, ref, what + " fused")
            fx, dgt = _d(2)
            before = _launches(c.core)
            L.check(c.core.lbfgsx_trial(c.h, oid, step0, C.byref(fx), C.byref(dgt)))
            assert _launches(c.core) == before and _ahead(c) == (runs0 + 1, hits0 + 1)  # handed out ahead: no launch
            _bits(c.down(L.VEC_G), g0, what + ": g at xp is left alone")
            _dot_ok(dg.value, g0, d, dt, what + ": g.d")
            assert sm.value == R.step_max_ref(x, d, lb, ub), what
            _sum_ok(fx.value, ref[1], dt, what + ": f trial")
            _dot_ok(dgt.value, ref[0], d, dt, what + ": grad(x).d")


@pytest.mark.parametrize("dtype", [O.F64, O.F32], ids=["f64", "f32"])
def test_softmax_partials_and_gradient_from_the_devices_own_w(A, dtype):
    """exp and log are not rounded by numpy as by the device, so w and v are held to numpy's within 8 ulps of the largest
    magnitude involved (each is a few operations on exp values in [0, 1] and on log(s) + m), while everything downstream of w
    is exact: the partials and the gradient from the w the device wrote, bit for bit"""
    P = _problem("f65", dtype)
    keep = []
    with Ctx(A, dtype, P.n) as c:
        L, dt = c.L, c.dt
        x = (0.3 * np.random.default_rng(9).standard_normal(P.n)).astype(dt)
        c.up(L.VEC_X, x)
        for with_ridge in (False, True):
            oid, lanes_used = _bind(c, P, SOFTMAX, P.labels, MR.RIDGE if with_ridge else None, 0, keep)
            fx, g2, x2 = _d(3)
            L.check(c.core.lbfgsx_eval(c.h, oid, C.byref(fx), C.byref(g2), C.byref(x2)))
            w, v, part = _read(c, P)
            Z = P.z(x, lanes_used).astype(np.float64)
            y = P.labels.astype(np.int64)
            lse = np.logaddexp.reduce(Z, axis=1)
            Wn = P.c1 * (np.exp(Z - lse[:, None]) - (np.arange(P.D)[None, :] == y[:, None]))
            vn = P.c1 * (lse - Z[np.arange(P.R), y])
            eps = float(np.finfo(dt).eps)
            assert np.abs(w - Wn).max() <= 8 * eps * P.c1 and np.abs(v - vn).max() <= 8 * eps * P.c1 * max(1.0, np.abs(Z).max())
            _bits(part, DR.partials(P.A, w, P.C), "part from the device's w")
            psi = LR.ridge(x, P.c0)[0].reshape(P.F, P.D) if with_ridge else None
            _bits(c.down(L.VEC_G), DR.gradient(part, psi).reshape(-1), "g from the device's partials")
            terms = np.concatenate([v, LR.ridge(x, P.c0)[1]]) if with_ridge else v
            _sum_ok(fx.value, terms, dt, "f from the device's v")


# ---------------------------------------------------------------- the same bits as the sparse forms
def _capture(body_returning_value, D):
    """the row body, with dz and its value also stored into the caller's device arrays p1 (R*D) and p2 (R): what the sparse
    forms' w and v hold, which their ABI does not read back"""
    z = "dz[k]" if D else "dz"
    idx = "r * D + k" if D else "r"
    loop = "for (int k = 0; k < D; k++) " if D else ""
    return ("const T value = [&]() -> T {%s\n}();\n%sconst_cast<T*>(p1)[%s] = %s;\nconst_cast<T*>(p2)[r] = value;\nreturn value;"
            % (body_returning_value, loop, idx, z))


SCALAR_SQUARE = "const T u = z - p0[r]; dz = u + c[1] * (u * u); return T(0.5) * (u * u);"
DENSE_SQUARE = "const T u = z[0] - p0[r]; dz[0] = u + c[1] * (u * u); return T(0.5) * (u * u);"


@pytest.mark.parametrize("dtype", [O.F64, O.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("R_,F,D,lanes", [(300, 37, 3, 0), (4097, 5, 2, 0), (4097, 5, 1, 4), (700, 65, 1, 0)],
                         ids=["short-D3", "long-D2", "long-D1-lanes4", "short-D1"])
def test_full_csr_through_the_sparse_forms_gives_the_same_bits(A, dtype, R_, F, D, lanes):
    """the same matrix as CSR with every entry stored, the same lanes: w, v and f bit for bit (R = 4097 puts every column of the
    sparse side on its long-column path, C = 4096); the gradients are two orders of one sum over the same rounded products
    A[r,j]*w[r,c], so they differ by at most 2 gamma_R sum_r |A[r,j] w[r,c]| per coordinate, gamma_k = k u / (1 - k u)"""
    import torch
    from lbfgspp_amd import _lib as LIB
    dt = NPDT[dtype]
    P = DR.Problem(R_, F, D, dt, seed=50 + R_ + D)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(P.n).astype(dt)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    lam = 0.25
    out = {}
    for form in ("dense", "sparse"):
        p1, p2 = torch.full((P.R * D,), 7.0, dtype=tdt, device="cuda"), torch.full((P.R,), 7.0, dtype=tdt, device="cuda")
        data = (torch.from_numpy(P.targets).cuda(), p1, p2)
        kw = dict(coord_body=MR.RIDGE, data=data, scalars=(lam, P.c1), lanes=lanes)
        if form == "dense":
            f = A.DenseLinearObjective(_capture(MR.COUPLED if D > 1 else DENSE_SQUARE, D), P.A, D, **kw)
        elif D > 1:
            f = A.MultiLinearObjective(_capture(MR.COUPLED, D), P.csr(), F, D, **kw)
        else:
            f = A.LinearObjective(_capture(SCALAR_SQUARE, 0), P.csr(), F, **kw)
        assert f.info(dt)["scratch_bytes"] == 0
        # one evaluation: a solve that stops at its start point leaves f(x0) and the gradient norm of x0
        s = A.LBFGSSolver(A.LBFGSParam(m=3, epsilon=1e30, epsilon_rel=0, max_iterations=1), dtype=dt)
        xx = x.copy()
        niter, fx = s.minimize(f, xx)
        assert s.last.nfev == 1 and np.array_equal(xx, x)
        g = np.empty(P.n, dt)
        LIB.check(s._core.lbfgsx_download(s.ctx, LIB.VEC_G, _vp(g)))
        torch.cuda.synchronize()
        out[form] = (p1.cpu().numpy(), p2.cpu().numpy(), fx, g)
        if form == "dense":
            c_info = (C.c_int64 * 8)()
            assert s._core.lbfgsx_objective_dense_info(s.ctx, C.byref(c_info)) == 0
            w = np.empty((P.R, D), dt)
            v = np.empty(P.R, dt)
            assert s._core.lbfgsx_objective_dense_read(s.ctx, _vp(w), _vp(v), None) == 0
            _bits(w.reshape(-1), out[form][0], "the captured dz is the dense form's w")
            _bits(v, out[form][1], "the captured value is the dense form's v")
            L_used = c_info[3]
            assert L_used == (lanes or DR.lanes_rule(F))
    assert LR.lanes_rule(P.R, P.R * F) == DR.lanes_rule(F)
    _bits(out["dense"][0], out["sparse"][0], "w")
    _bits(out["dense"][1], out["sparse"][1], "v")
    assert out["dense"][2] == out["sparse"][2], "f"
    assert np.any(out["dense"][0] != 7.0) and np.any(out["dense"][3] != 0)
    u = float(np.finfo(dt).eps) / 2
    gamma = P.R * u / (1 - P.R * u)
    mag = np.abs(P.A.astype(np.float64)).T @ np.abs(out["dense"][0].astype(np.float64).reshape(P.R, D))
    diff = np.abs(out["dense"][3].astype(np.float64) - out["sparse"][3].astype(np.float64)).reshape(F, D)
    print("max |dg| %.3g, smallest bound %.3g" % (diff.max(), (2 * gamma * mag).min()))
    assert (diff <= 2 * gamma * mag).all()
    # and the dense gradient is the restatement's, from the captured w
    part = DR.partials(P.A, out["dense"][0].reshape(P.R, D), P.C)
    _bits(out["dense"][3], DR.gradient(part, LR.ridge(x, lam)[0].reshape(F, D)).reshape(-1), "g")


# ---------------------------------------------------------------- against the reference
def _fixture(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
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


def _densified(A, inst, k):
    """the instance of tests/cpp/linear_probe.cpp (no "D") or multilinear_probe.cpp with its matrix dense: entries of a row
    that share a column add up (all are multiples of 1/4: the sums are exact)"""
    R_, D = inst["R"], inst.get("D", 1)
    F = inst["F"] if "D" in inst else inst["n"]
    r, j = np.arange(R_)[:, None], np.arange(k["per"])[None, :]
    col = (7 * r + 3 * j * j + j) % F
    val = ((31 * r + 17 * j) % 13 - 6) / 4.0
    dense = np.zeros((R_, F))
    np.add.at(dense, (np.broadcast_to(r, col.shape), col), val)
    n = F * D
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    x0 = k["amp"] * ((0.5 - t) * (1.0 + t))
    r = r.reshape(-1)
    if "D" in inst:
        y = ((5 * r) % D).astype(np.float64)
        b = (((11 * r[:, None] + 5 * np.arange(D)[None, :]) % 7 - 3) / 2.0).reshape(-1)
        hinge, square = MR.MHINGE, SQUARES
    else:
        y, b = np.where((5 * r) % 3 == 0, -1.0, 1.0), ((11 * r) % 7 - 3) / 2.0
        hinge, square = MR.scalar_body(LR.HINGE), MR.scalar_body(LR.SQUARE)
    if inst["solver"] == "lbfgs":
        return A.DenseLinearObjective(hinge, dense, D, coord_body=LR.RIDGE, data=(y,), scalars=(k["c0"],)), x0
    return A.DenseLinearObjective(square, dense, D, data=(b,)), x0


_INSTANCES = [(name, i) for name in ("linear_golden.json", "multilinear_golden.json") for i in _fixture(name)["instances"]]


@pytest.mark.parametrize("name,inst", _INSTANCES,
                         ids=lambda v: v.split("_")[0] if isinstance(v, str) else "%s-%dx%d" % (v["solver"], v["R"], v["n"]))
def test_densified_instances_follow_the_reference(A, name, inst):
    """every recorded iteration of every instance: the fixtures keep only iterations over which two accumulation orders of the
    reference agree to a tenth of their tolerance, which is what entitles a third order to be held to them"""
    n, tol = inst["n"], 1e-10
    assert inst["iterations"] >= 8
    f, x0 = _densified(A, inst, _fixture(name)["constants"])
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


# ---------------------------------------------------------------- convergence
@pytest.mark.parametrize("solver", ["lbfgs", "lbfgsb"])
def test_softmax_regression_converges(A, solver):
    """f = (1/R) sum_r (logsumexp(Z[r, :]) - Z[r, y_r]) + lam/2 |x|^2, R = 600, F = 20 (an intercept column of ones among them),
    D = 4, f64.  The solve ends on the gradient criterion; at the returned x the restatement (row sums, partials and gradient of
    dense_ref, the body's numpy twin dense_ref.softmax) gives the returned f -- the correctly rounded sum of its term values -- and a gradient on
    which the criterion's own inequality holds: ||g|| <= eps max(1, ||x||) for L-BFGS, the same on the infinity norm of the
    projected gradient for L-BFGS-B.  eps = 1e-6 as in the sparse forms' tests: at 1e-8 the decrease falls under the spacing
    of f"""
    R_, F, D, eps, lam = 600, 20, 4, 1e-6, 1e-2
    rng = np.random.default_rng(81)
    dense = rng.standard_normal((R_, F))
    dense[:, 0] = 1.0
    y = np.argmax(dense @ rng.standard_normal((F, D)) + 0.5 * rng.standard_normal((R_, D)), axis=1)
    f = A.DenseLinearObjective(SOFTMAX, dense, D, coord_body=MR.RIDGE, data=(y.astype(np.float64),), scalars=(lam, 1.0 / R_))
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
    Z = DR.row_sums(dense, X, DR.lanes_rule(F))
    W, v = DR.softmax(Z, y.astype(np.float64), 1.0 / R_)
    pg, pv = LR.ridge(x, lam)
    g = DR.gradient(DR.partials(dense, W), pg.reshape(F, D)).reshape(-1)
    f_ref = math.fsum(np.concatenate([v, pv]))
    bound = eps * max(1.0, float(np.linalg.norm(x)))
    measure = float(np.linalg.norm(g)) if solver == "lbfgs" else float(np.abs(g).max())
    print("%s: niter %d nfev %d fx %r (restatement %r) stopping measure %.6g (bound %.6g)" % (solver, niter, s.last.nfev, fx, f_ref,
                                                                                             measure, bound))
    assert measure <= bound
    assert fx == f_ref
    assert np.any(X[0] != 0)  # the intercepts moved


# ---------------------------------------------------------------- a device matrix is used in place
def test_device_matrix_is_used_in_place_and_a_host_matrix_is_copied(A):
    import torch
    R_, F, D = 4096, 2048, 2  # R*F*8 = 64 MiB: what a copy of the matrix takes, far above the allocator's granule
    P = DR.Problem(R_, F, D, np.float64, seed=77)
    x = np.random.default_rng(3).standard_normal(P.n)
    t = torch.from_numpy(np.ascontiguousarray(P.A)).cuda()
    host = np.ascontiguousarray(P.A).copy()
    torch.cuda.synchronize()
    with Ctx(A, O.F64, P.n) as c:
        L = c.L
        c.up(L.VEC_X, x)
        h = _compile(c, D, MR.COUPLED, MR.RIDGE)
        dev = C.c_void_p()
        L.check(c.core.lbfgsx_objective_upload_count(c.h, 0, _vp(P.targets), P.targets.size, C.byref(dev)))
        ptrs = (C.c_void_p * 4)()
        ptrs[0] = dev.value
        cs = (C.c_double * 8)(P.c0, P.c1, *([0.0] * 6))

        def bind(aptr, on_device):
            free0 = torch.cuda.mem_get_info()[0]
            L.check(c.core.lbfgsx_objective_bind_dense(c.h, h, R_, aptr, F, on_device, 0, C.byref(ptrs), C.byref(cs), None))
            return free0 - torch.cuda.mem_get_info()[0]

        def evaluate():
            fx, g2, x2 = _d(3)
            L.check(c.core.lbfgsx_eval(c.h, L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)))
            return fx.value, c.down(L.VEC_G).copy()
        L.check(c.core.lbfgsx_objective_bind(c.h, None, None, None, None))  # nothing bound: both binds allocate from the same state
        grown_host = bind(_vp(host), 0)
        assert _info(c)["own"] == 1 and _info(c)["lda"] == F
        f_host, g_host = evaluate()
        host[:] = 0.0  # the caller's host matrix is not read again
        assert evaluate()[0] == f_host
        L.check(c.core.lbfgsx_objective_bind(c.h, None, None, None, None))
        grown_dev = bind(C.c_void_p(t.data_ptr()), 1)
        assert _info(c)["own"] == 0
        # the device bind allocates w, v and the partials only (under 1 MiB): a whole matrix less than the host bind, up to the
        # allocator's granule
        print("context memory grown by %d (host matrix) and %d (device matrix) bytes" % (grown_host, grown_dev))
        assert grown_host - grown_dev >= R_ * F * 8 - (4 << 20) and grown_dev <= (4 << 20)
        f_dev, g_dev = evaluate()
        assert f_dev == f_host
        _bits(g_dev, g_host, "g from the device matrix")
        _bits(g_dev, P.evaluate(x, 64, "coupled", True)[0], "g against the restatement")
        t[:, 0] *= 2.0  # the caller's tensor IS the matrix
        torch.cuda.synchronize()
        f_mod, g_mod = evaluate()
        assert f_mod != f_dev and np.any(g_mod != g_dev)
        P2 = DR.Problem(R_, F, D, np.float64, seed=77)
        P2.A[:, 0] *= 2.0
        _bits(g_mod, P2.evaluate(x, 64, "coupled", True)[0], "g after the caller changed its tensor")


def test_python_class_takes_numpy_arrays_and_device_tensors_and_refuses_by_name(A):
    import torch
    P = DR.Problem(300, 40, 3, np.float64, seed=12)
    x0 = np.random.default_rng(6).standard_normal(P.n)
    out = []
    padded = torch.zeros((P.R, P.F + 8), dtype=torch.float64, device="cuda")
    padded[:, :P.F] = torch.from_numpy(np.ascontiguousarray(P.A)).cuda()
    for m in (P.A, padded[:, :P.F]):
        f = A.DenseLinearObjective(MR.MHINGE, m, P.D, coord_body=MR.RIDGE, data=(P.labels,), scalars=(0.1,))
        assert f.on_device == (m is not P.A) and f.n == P.n and f.lda == (P.F if m is P.A else P.F + 8)
        s = A.LBFGSSolver(A.LBFGSParam(m=5, epsilon=0, epsilon_rel=0, max_iterations=8), linesearch=A.LS_MORE_THUENTE)
        x = x0.copy()
        niter, fx = s.minimize(f, x)
        out.append((niter, s.last.nfev, fx, x))
    assert out[0][:3] == out[1][:3] and out[0][0] == 8
    _bits(out[1][3], out[0][3], "x from a device tensor with a row stride")
    with pytest.raises(ValueError, match="strides \\(1, 48\\)"):
        A.DenseLinearObjective(MR.MHINGE, padded.t(), P.D)
    with pytest.raises(ValueError, match="dtype torch.float16"):
        A.DenseLinearObjective(MR.MHINGE, padded.half(), P.D)
    f32 = A.DenseLinearObjective(MR.MHINGE, padded[:, :P.F].float(), P.D, data=(P.labels,))
    with pytest.raises(ValueError, match="dtype torch.float32 and the solver torch.float64"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(f32, x0.copy())


# ---------------------------------------------------------------- accounting
def test_lbfgsb_first_trials_all_ride_on_the_dg_maxstep_pass(A):
    """multi-target non-negative least squares, bounds active at the start and at the end: 25 iterations, 25 first trials
    evaluated by lbfgsx_b_dg_maxstep_trial and handed out without a launch"""
    core, _ = A.load()
    R_, F, D, iters = 300, 20, 3, 25
    rng = np.random.default_rng(80)
    dense = rng.standard_normal((R_, F))
    B = dense @ rng.standard_normal((F, D))
    f = A.DenseLinearObjective(SQUARES, dense, D, data=(B.reshape(-1),))
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
    assert niter == iters and (ahead[0], ahead[1]) == (iters, iters)
    assert fx < f0 and (x >= 0).all() and (x == 0).any() and (x > 0).any()
    r = dense @ x.reshape(F, D) - B
    assert abs(fx - 0.5 * float((r * r).sum())) <= 1e-10 * max(1.0, fx)


# ---------------------------------------------------------------- refusals
def _nothing_bound(c):
    fx, g2, x2 = _d(3)
    before = _launches(c.core)
    assert c.core.lbfgsx_eval(c.h, c.L.OBJ_BOUND, C.byref(fx), C.byref(g2), C.byref(x2)) != 0
    assert _launches(c.core) == before
    assert c.core.lbfgsx_objective_dense_info(c.h, None) == c.L.E_INVALID
    assert c.core.lbfgsx_objective_dense_read(c.h, None, None, None) == c.L.E_INVALID


def test_offending_requests_are_refused_by_value_and_nothing_is_evaluated(A):
    n, D = 6, 3  # F = 2
    name = "dense linear-model objective"
    mat = np.arange(6.0).reshape(3, 2)
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0]))
    with Ctx(A, O.F64, n) as c:
        L = c.L
        h = _compile(c, D, MR.MHINGE)
        others = {}
        log = C.create_string_buffer(4096)
        for key, fn, args in (("multi", c.core.lbfgsx_objective_compile_linear_multi, (D, None, MR.MHINGE.encode())),
                              ("scalar", c.core.lbfgsx_objective_compile_linear, (None, LR.HINGE.encode())),
                              ("term", c.core.lbfgsx_objective_compile, (1, b"g[0] = x[0]; return T(0.5) * (x[0] * x[0]);"))):
            others[key] = C.c_void_p()
            assert fn(C.byref(others[key]), c.dtype, *args, log, len(log)) == 0, log.value.decode()

        def bind(handle=h, R_=3, aptr=_vp(mat), lda=2, lanes=0, oid=None):
            return c.core.lbfgsx_objective_bind_dense(c.h, handle, R_, aptr, lda, 0, lanes, None, None, oid)
        for kw, what in ((dict(R_=0), "R = 0: a dense linear-model objective has at least one row"),
                         (dict(R_=-4), "R = -4: a dense linear-model objective has at least one row"),
                         (dict(aptr=None), "A is null"),
                         (dict(lda=1), "lda = 1 is less than F = n / D = 2"),
                         (dict(R_=2 ** 31), "R = 2147483648 exceeds 2^31 - 1 = 2147483647"),
                         (dict(lanes=3), "lanes = 3: the lanes that share a row are 0 (by the rule) or a power of two in 1..64"),
                         (dict(lanes=128), "lanes = 128"), (dict(lanes=-1), "lanes = -1")):
            assert bind() == 0  # something is bound before each refusal
            before = _launches(c.core)
            rc = bind(oid=C.byref(C.c_int(-1)), **kw)
            assert rc == L.E_INVALID and name + ": " + what in L.last_error(), L.last_error()
            assert _launches(c.core) == before
            _nothing_bound(c)
        # handles of the other forms
        for key, noun in (("multi", "multi-output linear-model objective"), ("scalar", "linear-model objective"), ("term", "term objective")):
            assert bind() == 0
            assert bind(handle=others[key]) == L.E_INVALID
            assert "lbfgsx_objective_bind_dense: the handle is a %s, not a %s (lbfgsx_objective_compile_dense)" % (noun, name) \
                in L.last_error(), L.last_error()
            _nothing_bound(c)
        # the other bind calls refuse a dense handle
        oid = C.c_int(-1)
        assert bind(oid=C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND and _info(c)["D"] == D
        assert c.core.lbfgsx_objective_bind(c.h, h, None, None, None) == L.E_INVALID
        assert "a %s is bound with its matrix: lbfgsx_objective_bind_dense" % name in L.last_error()
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
        assert c.core.lbfgsx_objective_bind_linear(c.h, h, 1, 1, _vp(one[0]), _vp(one[1]), _vp(one[2]), 0, 0, None, None,
                                                   None) == L.E_INVALID
        assert "the handle is a %s, not a linear-model objective" % name in L.last_error()
        _nothing_bound(c)
        # a sparse form bound after a dense one, and back: each frees the other's arrays
        assert c.core.lbfgsx_objective_bind_linear(c.h, others["scalar"], 1, 1, _vp(one[0]), _vp(one[1]), _vp(one[2]), 0, 0, None,
                                                   None, None) == 0
        assert c.core.lbfgsx_objective_dense_info(c.h, None) == L.E_INVALID
        assert bind() == 0 and _info(c)["R"] == 3
        for v in others.values():
            c.core.lbfgsx_objective_destroy(v)
    # n % D != 0: both values named, no launch
    with Ctx(A, O.F64, 7) as c:
        L = c.L
        h = _compile(c, D, MR.MHINGE)
        before = _launches(c.core)
        rc = c.core.lbfgsx_objective_bind_dense(c.h, h, 3, _vp(mat), 2, 0, 0, None, None, None)
        assert rc == L.E_INVALID and name + ": n = 7 is not a multiple of D = 3" in L.last_error(), L.last_error()
        assert _launches(c.core) == before
        _nothing_bound(c)


def test_refused_modes_say_so(A):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    P = DR.Problem(50, 16, 4, np.float64, seed=13)
    f = A.DenseLinearObjective(MR.MHINGE, P.A, P.D, coord_body=MR.RIDGE, data=(P.labels,), scalars=(0.1,))
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
