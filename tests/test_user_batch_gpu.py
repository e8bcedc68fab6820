"""GPU suite: a caller-supplied objective over the lock-step batch (lbfgsx_lockstep_minimize_fn, LockstepBatch.minimize_fn)
and the two launches it adds, lbfgsx_bat_pack / lbfgsx_bat_unpack (csrc/batched_user.hip)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1
    return A


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Desc(C.Structure):  # lbfgsx_bat_desc (include/lbfgsx.h)
    _fields_ = [("active", C.c_int), ("mode", C.c_int), ("x_in", C.c_int), ("x_out", C.c_int), ("col_u", C.c_int),
                ("col_w", C.c_int), ("i_num", C.c_int), ("i_den", C.c_int), ("i_num2", C.c_int), ("i_theta", C.c_int),
                ("i_out", C.c_int), ("pad", C.c_float), ("step", C.c_double)]


def _bind(core):
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    for name, res, args in (("lbfgsx_bat_create", i32, [C.POINTER(vp), i32, i64, i32, i32, i32]), ("lbfgsx_bat_destroy", None, [vp]),
                            ("lbfgsx_bat_vec", vp, [vp, i32, i32, i32]), ("lbfgsx_bat_ld", i64, [vp]), ("lbfgsx_bat_sync", i32, [vp]),
                            ("lbfgsx_bat_scalar_index", i32, [vp, i32, i32]), ("lbfgsx_bat_launch", i32, [vp, i32, i32, vp, i32, vp]),
                            ("lbfgsx_bat_packed", vp, [vp, i32]), ("lbfgsx_bat_pack", i32, [vp, vp]),
                            ("lbfgsx_bat_unpack", i32, [vp, vp, vp])):
        f = getattr(core, name)
        f.restype, f.argtypes = res, args


@pytest.mark.parametrize("dtype,n,P", [(np.float32, 1003, 7), (np.float64, 4097, 5), (np.float32, 250000, 4), (np.float64, 60000, 3),
                                       (np.float32, 4096, 300)])
def test_pack_and_unpack_equal_the_statements_they_replace_bit_for_bit(A, torch, dtype, n, P):
    """problems in different point slots, different steps, some sitting out, packed rows in another order than the problems:
    the point slot and the packed row after lbfgsx_bat_pack are the bytes LBFGSX_BAT_POINT writes; the gradient slot after
    lbfgsx_bat_unpack is the packed row, and its grad . drt is LBFGSX_BAT_GDOT's on the same gradient, bit for bit.  n not a
    multiple of the 16-byte vector width, and n beyond one block's share (250 000 floats), included."""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    _bind(core)
    dt = L.F64 if dtype == np.float64 else L.F32
    bat = C.c_void_p()
    L.check(core.lbfgsx_bat_create(C.byref(bat), dt, n, 4, P, 0))
    try:
        ld = core.lbfgsx_bat_ld(bat)
        OUT0 = core.lbfgsx_bat_scalar_index(bat, 3, 0)
        gen = torch.Generator(device="cuda:0").manual_seed(n + P)
        tdt = torch.float64 if dtype == np.float64 else torch.float32

        def view(kind, point):  # [P, n] view of a slot (kind 2: the directions)
            return L.device_tensor(core.lbfgsx_bat_vec(bat, kind, point, 0), (P, n), dtype, 0, row_stride=ld)

        def packed(kind):
            return L.device_tensor(core.lbfgsx_bat_packed(bat, kind), (P, n), dtype, 0, row_stride=ld)

        for pt in range(3):
            view(0, pt).copy_(torch.randn(P, n, generator=gen, device="cuda:0", dtype=tdt))
        view(2, 0).copy_(torch.randn(P, n, generator=gen, device="cuda:0", dtype=tdt))
        rng = np.random.default_rng(P)
        active = [p for p in range(P) if p % 4 != 1]
        rows = rng.permutation(len(active))
        desc = (Desc * P)()
        for d in desc:
            d.i_out = OUT0
        for k, p in enumerate(active):
            d = desc[p]
            d.active, d.x_in, d.x_out, d.col_u, d.step = 1, p % 3, (p % 3 + 1 + (p // 3) % 2) % 3, int(rows[k]), float(rng.uniform(1e-3, 2.0))
        torch.cuda.synchronize()
        before = [view(0, pt).clone() for pt in range(3)]
        # the statements replaced: POINT, then (gradient put into the slot by the caller) GDOT
        L.check(core.lbfgsx_bat_launch(bat, 4, -1, desc, 0, None))
        L.check(core.lbfgsx_bat_sync(bat))
        want_x = [view(0, pt).clone() for pt in range(3)]
        grads = torch.randn(P, n, generator=gen, device="cuda:0", dtype=tdt)
        for p in active:
            view(1, desc[p].x_out)[p].copy_(grads[p])
        torch.cuda.synchronize()
        want_dg = np.full(P, np.nan)
        L.check(core.lbfgsx_bat_launch(bat, 5, -1, desc, 1, want_dg.ctypes.data_as(C.c_void_p)))
        # ... and the two launches
        for pt in range(3):
            view(0, pt).copy_(before[pt])
            view(1, pt).zero_()
        packed(0).fill_(float("nan"))
        torch.cuda.synchronize()
        L.check(core.lbfgsx_bat_pack(bat, desc))
        L.check(core.lbfgsx_bat_sync(bat))
        UX, UG = packed(0), packed(1)

        def same_bytes(u, v):
            return torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))

        for pt in range(3):
            assert same_bytes(view(0, pt), want_x[pt]), pt
        for p in active:
            assert same_bytes(UX[desc[p].col_u], want_x[desc[p].x_out][p]), p
            UG[desc[p].col_u].copy_(grads[p])
        torch.cuda.synchronize()
        got_dg = np.full(P, np.nan)
        L.check(core.lbfgsx_bat_unpack(bat, desc, got_dg.ctypes.data_as(C.c_void_p)))
        L.check(core.lbfgsx_bat_sync(bat))
        assert got_dg.tobytes() == want_dg.tobytes() and np.all(np.isfinite(got_dg[active]))
        for p in range(P):
            for pt in range(3):
                expect = grads[p] if (p in active and desc[p].x_out == pt) else torch.zeros(n, device="cuda:0", dtype=tdt)
                assert same_bytes(view(1, pt)[p], expect), (p, pt)
        # malformed tables are refused before anything is launched
        for field, bad in (("x_out", 3), ("x_in", -1), ("col_u", P), ("col_u", -1), ("i_out", 1 << 20)):
            keep = getattr(desc[active[0]], field)
            setattr(desc[active[0]], field, bad)
            assert core.lbfgsx_bat_pack(bat, desc) == L.E_INVALID and core.lbfgsx_bat_unpack(bat, desc, got_dg.ctypes.data_as(C.c_void_p)) == L.E_INVALID
            setattr(desc[active[0]], field, keep)
        desc[active[0]].x_out = desc[active[0]].x_in
        assert core.lbfgsx_bat_pack(bat, desc) == L.E_INVALID
        if len(active) > 1:
            desc[active[0]].x_out = (desc[active[0]].x_in + 1) % 3
            desc[active[0]].col_u = desc[active[1]].col_u
            assert core.lbfgsx_bat_pack(bat, desc) == L.E_INVALID
    finally:
        core.lbfgsx_bat_destroy(bat)


def rosen_row(torch):
    """the single-problem callable of tests/test_user_objective_gpu.py: the reference's example-rosenbrock.cpp"""
    def fn(x, g):
        x0, x1 = x[0::2], x[1::2]
        t1 = 1.0 - x0
        t2 = 10.0 * (x1 - x0 * x0)
        g1 = 20.0 * t2
        g[1::2] = g1
        g[0::2] = -2.0 * (x0 * g1 + t1)
        return float((t1 * t1 + t2 * t2).sum(dtype=torch.float64))
    return fn


def by_rows(single):
    """the batch callable whose per-row arithmetic IS the single-problem callable's (f row by row: the claim under test is the
    library's, not that torch's row-wise sum equals its 1-D sum)"""
    def fn(ids, X, G):
        return [single(X[k], G[k]) for k in range(len(ids))]
    return fn


@pytest.mark.parametrize("ls", [O.LS_MT, O.LS_NW])
@pytest.mark.parametrize("dtype,n,count,m,iters", [(np.float32, 20000, 6, 5, 12), (np.float64, 5000, 5, 7, 15),
                                                   (np.float32, 3002, 3, 4, 8), (np.float32, 120000, 3, 4, 6)])
def test_every_member_follows_its_stand_alone_solve_bit_for_bit(A, torch, ls, dtype, n, count, m, iters):
    """niter, nfev, fx and the final x of every problem equal LBFGSSolver.minimize(DeviceObjective(...)) on that problem
    exactly: the same torch arithmetic for f and grad, the library's reductions for everything else.  No problem is left out;
    one whose stand-alone solve raises carries that status in the batch.  n = 3002 floats: the statement-wise driver (no one-launch
    iteration for an n off the vector width); n = 120 000 floats: problems split over two blocks."""
    from lbfgspp_amd import batched as B
    par = A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters)
    dt = O.F64 if dtype == np.float64 else O.F32
    x0 = np.stack([O.rosen_x0(n, 40 + p, dt) for p in range(count)])
    single = rosen_row(torch)
    batch = B.LockstepBatch(par, n, count, dtype=dtype, linesearch=ls)
    recs, xs = batch.minimize_fn(by_rows(single), x0, return_x=True)
    st = batch.stats
    batch.close()
    assert st["fused"] == (n % (4 if dtype == np.float32 else 2) == 0) and st["user_calls"] >= 2
    for p in range(count):
        s = A.LBFGSSolver(par, linesearch=ls, dtype=dtype)
        x = x0[p].copy()
        status = 0
        try:
            s.minimize(A.DeviceObjective(single), x)
        except (RuntimeError, ArithmeticError, ValueError):
            status = s.last.status
        assert (recs["nfev"][p], recs["status"][p]) == (s.last.nfev, status), p
        if status == 0:
            assert (recs["niter"][p], recs["fx"][p], recs["gnorm"][p]) == (s.last.niter, s.last.fx, s.last.gnorm), p
        assert np.array_equal(xs[p], x), p


def quad_rows(torch, a, b, log=None):
    at, bt = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(b, device="cuda:0")

    def fn(ids, X, G):
        if log is not None:
            log.append(ids.copy())
        sel = torch.as_tensor(ids, device="cuda:0")
        aa, bb = at[sel], bt[sel]
        r = aa * X - bb
        torch.mul(aa, r, out=G)
        return [0.5 * float((r[k] * r[k]).sum(dtype=torch.float64)) for k in range(len(ids))]
    return fn


def test_membership_and_user_data_in_a_batch(A, torch):
    """`count` diagonal quadratics with the caller's a, b, x0 (nothing seed-generated) of very different condition: the
    minimisers are b / a to epsilon; a problem is listed once per evaluation it needs and never after it has converged, nact
    shrinks accordingly; and what the others do does not depend on who else is in the batch (a sub-batch gives the same
    records and iterates)."""
    from lbfgspp_amd import batched as B
    n, count, eps = 6000, 8, 1e-7
    rng = np.random.default_rng(11)
    kappa = [1.0, 1.0, 4.0, 30.0, 100.0, 2.0, 200.0, 60.0]
    a = np.stack([1.0 + (k - 1.0) * rng.random(n) for k in kappa])
    b = rng.standard_normal((count, n))
    x0 = rng.standard_normal((count, n))
    par = A.LBFGSParam(m=6, epsilon=eps, epsilon_rel=0.0, max_iterations=5000)  # (a cap: condition numbers <= 200 need far fewer)
    log = []
    batch = B.LockstepBatch(par, n, count, dtype=np.float64)
    recs, xs = batch.minimize_fn(quad_rows(torch, a, b, log), torch.as_tensor(x0, device="cuda:0"), return_x=True)
    assert batch.stats["user_calls"] == len(log)
    batch.close()
    assert np.all(recs["status"] == 0) and np.all(recs["niter"] < 5000) and np.all(recs["gnorm"] <= eps)
    assert np.abs(xs - b / a).max() <= eps  # a >= 1: |x - b/a| <= |grad|
    assert list(log[0]) == list(range(count))
    for ids in log:
        assert np.all(np.diff(ids) > 0)
    appear = np.bincount(np.concatenate(log), minlength=count)
    assert np.array_equal(appear, recs["nfev"])
    assert len(log[-1]) < count and recs["nfev"].max() > 3 * recs["nfev"].min()
    last = [max(i for i, ids in enumerate(log) if p in ids) for p in range(count)]
    assert len(set(last)) > 2  # they left at different times
    sub = [1, 4, 6]
    small = B.LockstepBatch(par, n, len(sub), dtype=np.float64)
    r2, x2 = small.minimize_fn(quad_rows(torch, a[sub], b[sub]), x0[sub], return_x=True)
    small.close()
    assert np.array_equal(r2, recs[sub]) and np.array_equal(x2, xs[sub])


def test_a_failing_callback_fails_the_call_and_leaves_the_handle_usable(A, torch):
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    n, count = 8000, 4
    par = A.LBFGSParam(m=4, epsilon=0.0, epsilon_rel=0.0, max_iterations=8)
    x0 = np.stack([O.rosen_x0(n, 90 + p, O.F32) for p in range(count)])
    good = by_rows(rosen_row(torch))
    calls = [0]

    def bad(ids, X, G):
        calls[0] += 1
        if calls[0] == 3:
            raise KeyError("third call")
        return good(ids, X, G)

    fresh = B.LockstepBatch(par, n, count, dtype=np.float32)
    want, xw = fresh.minimize_fn(good, x0, return_x=True)
    want_b, xwb = fresh.minimize(first=3, seed_base=5, return_x=True)
    fresh.close()
    batch = B.LockstepBatch(par, n, count, dtype=np.float32)
    with pytest.raises(KeyError, match="third call"):
        batch.minimize_fn(bad, x0, return_x=True)
    assert batch.status == L.E_USER
    got, xg = batch.minimize_fn(good, x0, return_x=True)
    got_b, xgb = batch.minimize(first=3, seed_base=5, return_x=True)
    batch.close()
    assert np.array_equal(got, want) and np.array_equal(xg, xw)
    assert np.array_equal(got_b, want_b) and np.array_equal(xgb, xwb)
    # a C callback that simply returns non-zero: LBFGSX_E_USER and a message, no exception object involved
    _, sol = A.load()
    batch = B.LockstepBatch(par, n, count, dtype=np.float32)
    items = (L.BatchItem * count)()
    err = C.create_string_buffer(256)
    rc = sol.lbfgsx_lockstep_minimize_fn(batch._h, x0.ctypes.data_as(C.c_void_p), L.BATCH_OBJECTIVE_FN(lambda *a: 7), None, items,
                                         None, None, err, 256)
    batch.close()
    assert rc == L.E_USER and b"returned 7" in err.value
