"""GPU suite: the recursion's last step inside the next search's first trial (k_trial_last, PersistArgs::defer_last,
lbfgsx_last_in_trial_request).

A persistent launch from the gradient ends with step 2c-1; the first trial of the next search forms d = q + (alpha_0 - beta) s_0
in its own pass with the expression of the step kernels and returns grad.d with fx and dg; every other reader of d runs the step
as a step launch first.  Same statements on the same operands, so every run with the form on (the default) is compared bit
for bit -- np.array_equal -- with the same run under LBFGSX_LAST_IN_TRIAL=0.

Extended Rosenbrock needs an even dimension, so its sizes are the even neighbours of the odd ones a scalar tail asks for: with
four floats per 16-byte vector they still leave a tail of two in f32.  The f64 tail (one element) can only occur with the
diagonal quadratic, which therefore runs the same comparison under More-Thuente at the odd sizes."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

# elements of q a persistent launch keeps on the CUs of an MI355X: 45 slots x 512 blocks x 256 threads x 16 bytes
RESIDENT = {O.F64: 11_796_480, O.F32: 23_592_960}


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


def _counts(core, h, name="lbfgsx_last_in_trial_counts"):
    """last step: {launches that ended one step early, steps run by a first trial, steps run on their own, form enabled};
    lbfgsx_post_in_trial_counts: {post-form trials issued, accepted, launches from the gradient, form enabled}"""
    out = (C.c_int64 * 4)()
    assert getattr(core, name)(h, C.byref(out)) == 0
    return tuple(int(v) for v in out)


def _persist(core, h):
    out = (C.c_int64 * 4)()
    core.lbfgsx_persist_counts(h, C.byref(out))
    return tuple(int(v) for v in out)


def _down(core, L, h, which, n, dt):
    out = np.empty(n, dt)
    L.check(core.lbfgsx_download(h, which, out.ctypes.data_as(C.c_void_p)))
    return out


def _run(A, monkeypatch, switch, f, x0, dtype, m, iters, ls, at_iteration=None):
    """one solve: x, grad and the direction it leaves, its counts after every iteration; at_iteration(k, solver) runs in the
    iteration hook; an exception of the solve is returned, not raised"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    core.lbfgsx_persistent_resident_elems.restype = C.c_int64
    core.lbfgsx_persistent_resident_elems.argtypes = [C.c_void_p]
    monkeypatch.setenv("LBFGSX_LAST_IN_TRIAL", switch)
    gc.collect()
    dt, n = O.NPDT[dtype], x0.size
    s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters), linesearch=ls, dtype=dt)
    per_iter = []

    def hook(k):
        per_iter.append((_counts(core, s.ctx), _counts(core, s.ctx, "lbfgsx_post_in_trial_counts")))
        if at_iteration:
            at_iteration(k, s)

    s.set_iteration_hook(hook)
    x = x0.copy()
    error = None
    try:
        niter, fx = s.minimize(f, x)
    except ArithmeticError as e:
        niter, fx, error = -1, float("nan"), str(e)
    h = s.ctx
    before_download = _counts(core, h)
    out = dict(niter=niter, nfev=s.last.nfev, fx=fx, x=x, error=error, per_iter=per_iter, before_download=before_download,
               g=_down(core, L, h, L.VEC_G, n, dt), d=_down(core, L, h, L.VEC_D, n, dt), last=_counts(core, h),
               post=_counts(core, h, "lbfgsx_post_in_trial_counts"), persist=_persist(core, h),
               resident=int(core.lbfgsx_persistent_resident_elems(h)))
    s.close()
    del s
    gc.collect()
    return out


def _same_bits(on, off):
    assert (on["niter"], on["nfev"]) == (off["niter"], off["nfev"]) and on["fx"] == off["fx"]
    for v in ("x", "g", "d"):
        assert np.array_equal(on[v], off[v]), v
    assert on["post"] == off["post"] and len(on["per_iter"]) == len(off["per_iter"]) > 0
    assert off["last"] == (0, 0, 0, 0)
    assert on["persist"][1] == 0 and off["persist"][1] == 0   # no time-out


def _rejected_after_fused(run):
    """searches whose first trial ran the deferred step and was rejected: the step then ran again on its own, ahead of the
    second trial (both counts move within one iteration)"""
    prev, hits = (0, 0, 0, 1), 0
    for last, _ in run["per_iter"]:
        hits += int(last[1] == prev[1] + 1 and last[2] == prev[2] + 1)
        prev = last
    return hits


# (dtype, n, iterations): n = 4098 is just above LBFGSX_PERSIST_MIN_N and wholly resident; 1 048 582 ends in a partial tile;
# the third size has a streamed part past the resident slots.  The iteration counts are the first at which the run with the
# switch off shows a rejected post-form first trial behind an accepted one (lbfgsx_post_in_trial_counts: issued > accepted;
# the search of iteration 15 at n = 4098, of iteration 14 at the other sizes), in an iteration the hook still sees
ROSEN_CASES = [
    (O.F64, 4098, 16), (O.F32, 4098, 16),
    (O.F64, 1_048_582, 15), (O.F32, 1_048_582, 15),
    (O.F64, RESIDENT[O.F64] + 1024 * 3 + 2, 15), (O.F32, RESIDENT[O.F32] + 1024 * 5 + 6, 15),
]


@pytest.mark.parametrize("dtype,n,iters", ROSEN_CASES)
def test_rosenbrock_more_thuente_same_bits(A, monkeypatch, dtype, n, iters):
    """LBFGSSolver, extended Rosenbrock, More-Thuente, m = 3: x, grad, the downloaded direction (which runs a step still owed),
    niter, nfev and fx with the form on and off.  The run shows both a deferred step taken by a first trial and a step
    run on its own after a rejected first trial."""
    x0 = O.rosen_x0(n, 7, dtype)
    on, off = (_run(A, monkeypatch, sw, A.ExtendedRosenbrock(), x0, dtype, 3, iters, A.LS_MORE_THUENTE) for sw in ("1", "0"))
    print("last-step counts on:", on["last"], "post-form counts:", on["post"], "off:", off["post"],
          "rejected after fused:", _rejected_after_fused(on))
    _same_bits(on, off)
    deferred, fused, settled, enabled = on["last"]
    assert enabled == 1 and deferred >= 1 and fused >= 1
    assert off["post"][0] > off["post"][1]              # the instance has a rejected post-form first trial
    assert _rejected_after_fused(on) >= 1
    assert settled >= _rejected_after_fused(on)
    assert deferred == on["post"][2]                    # every launch from the gradient ended one step early
    if n > RESIDENT[dtype]:
        assert on["resident"] == RESIDENT[dtype]


@pytest.mark.parametrize("dtype,n", [(O.F64, 4099), (O.F32, 4099), (O.F64, RESIDENT[O.F64] + 1024 * 3 + 3),
                                      (O.F32, RESIDENT[O.F32] + 1024 * 5 + 5)])
def test_quadratic_more_thuente_same_bits_with_a_scalar_tail(A, monkeypatch, dtype, n):
    """The odd sizes, which only the diagonal quadratic can have: the scalar tail of the last form (one double, three or one
    floats), wholly resident and with a streamed part."""
    a, b = O.quad_problem(n, 10.0, 1, dtype)
    f, x0 = A.DiagQuadratic(a, b), np.zeros(n, O.NPDT[dtype])
    on, off = (_run(A, monkeypatch, sw, f, x0, dtype, 3, 8, A.LS_MORE_THUENTE) for sw in ("1", "0"))
    print("last-step counts on:", on["last"], "post-form counts:", on["post"])
    _same_bits(on, off)
    assert on["last"][0] >= 1 and on["last"][1] >= 1 and on["last"][0] == on["post"][2]


def test_quadratic_nocedal_wright_same_bits(A, monkeypatch):
    """n = 1e5 under Nocedal-Wright, a policy that gets grad.d before its search: no launch ends early, same bits."""
    n = 100_000
    a, b = O.quad_problem(n, 10.0, 1, O.F64)
    f, x0 = A.DiagQuadratic(a, b), np.zeros(n)
    on, off = (_run(A, monkeypatch, sw, f, x0, O.F64, 3, 12, A.LS_NOCEDAL_WRIGHT) for sw in ("1", "0"))
    _same_bits(on, off)
    assert on["last"] == (0, 0, 0, 1) and on["post"][2] >= 5


class _Manual:
    """The driver's statements through the C ABI, one search = one trial at a given step."""

    def __init__(self, A, monkeypatch, switch, request, n, m, a, b, x0):
        from lbfgspp_amd import _lib as L
        self.L, (self.core, _) = L, A.load()
        monkeypatch.setenv("LBFGSX_LAST_IN_TRIAL", switch)
        self.h = C.c_void_p()
        L.check(self.core.lbfgsx_create(C.byref(self.h), O.F64, n, m, 0, 0))
        self.n = n
        for which, v in ((L.VEC_A, a), (L.VEC_B, b), (L.VEC_X, x0)):
            L.check(self.core.lbfgsx_upload(self.h, which, np.ascontiguousarray(v, np.float64).ctypes.data_as(C.c_void_p)))
        L.check(self.core.lbfgsx_last_in_trial_request(self.h, request))
        r = [C.c_double() for _ in range(3)]
        L.check(self.core.lbfgsx_eval(self.h, O.OBJ_QUAD, *[C.byref(v) for v in r]))
        self.dg, self.pending = C.c_double(), C.c_int(0)
        L.check(self.core.lbfgsx_apply_Hv(self.h, L.VEC_G, -1.0, C.byref(self.dg)))

    def search(self, step, first=None):
        """one search (first: a first trial at that step which the search does not keep); returns what the trials gave"""
        L, core, h = self.L, self.core, self.h
        L.check(core.lbfgsx_ls_begin(h))
        L.check(core.lbfgsx_ls_post_in_trial(h, -1.0))
        got = []
        for t in ([first] if first is not None else []) + [step]:
            fx, dgt, dg0 = C.c_double(), C.c_double(), C.c_double()
            L.check(core.lbfgsx_trial_first(h, O.OBJ_QUAD, t, C.byref(fx), C.byref(dgt), C.byref(dg0)))
            got.append((fx.value, dgt.value, dg0.value))
        L.check(core.lbfgsx_ls_end(h, 0))
        return got

    def product(self):
        """the statements after a search; the direction's grad.d, or "pending" """
        L, core, h = self.L, self.core, self.h
        r = [C.c_double() for _ in range(4)]
        L.check(core.lbfgsx_post_linesearch_spec(h, -1.0, *[C.byref(v) for v in r]))
        assert r[2].value > np.finfo(np.float64).eps * r[3].value
        L.check(core.lbfgsx_commit_correction(h))
        L.check(core.lbfgsx_apply_Hv_pending(h, L.VEC_G, -1.0, C.byref(self.dg), C.byref(self.pending)))
        return self.pending.value, self.dg.value

    def down(self, which):
        return _down(self.core, self.L, self.h, which, self.n, np.float64)

    def counts(self):
        return _counts(self.core, self.h)

    def close(self):
        self.core.lbfgsx_destroy(self.h)


@pytest.mark.parametrize("n", [4099, RESIDENT[O.F64] + 1024 * 3 + 1])
def test_statement_level(A, monkeypatch, n):
    """Through the C ABI, against a context with the switch off.  After a product whose launch ended one step early:
    downloading d gives the bits of the full product; the grad.d that comes back with the first trial is the full product's
    stored grad.d; a rejected first trial is followed by the step on its own, and the second trial sees the same d."""
    m = 3
    a, b = O.quad_problem(n, 10.0, 1, O.F64)
    x0 = np.zeros(n)
    res = {}
    for sw in ("1", "0"):
        c = _Manual(A, monkeypatch, sw, 1, n, m, a, b, x0)
        L = c.L
        log = []
        c.search(1.0)
        log.append(c.product())                         # first product after a plain trial: a full launch
        c.search(1.0)                                   # post-form first trial, accepted
        log.append(c.product())                         # launch from the gradient: ends early with the switch on
        log.append(c.counts())
        log.append(c.search(1.0))                       # the first trial runs the step and returns grad.d
        log.append(c.counts())
        log.append(c.product())
        d_mid = c.down(L.VEC_D)                         # a download while the step is owed: it runs first
        log.append(c.counts())
        log.append(c.search(1.0))                       # the first trial still returns grad.d (the caller was told "pending")
        log.append(c.product())
        log.append(c.search(1.0, first=0.5))            # the first trial runs the step and is rejected; the second is plain
        log.append(c.counts())
        log.append(c.product())
        res[sw] = (log, d_mid, c.down(L.VEC_D), c.down(L.VEC_X), c.down(L.VEC_G))
        c.close()
    on, off = res["1"], res["0"]
    for k in (1, 2, 3, 4):
        assert np.array_equal(on[k], off[k])
    lon, loff = on[0], off[0]
    # products: (pending, grad.d)
    assert lon[0] == loff[0] and lon[0][0] == 0
    for k in (1, 5, 8):
        assert loff[k][0] == 0 and lon[k][0] == 1 and np.isnan(lon[k][1]), k
    assert lon[11] == loff[11] and lon[11][0] == 0      # behind a search that rejected its first trial: a full launch
    # counts: {ended early, run by a first trial, run on their own, enabled}
    assert lon[2] == (1, 0, 0, 1) and lon[4] == (1, 1, 0, 1) and lon[6] == (2, 1, 1, 1) and lon[10] == (3, 2, 2, 1)
    assert loff[10] == (0, 0, 0, 0)
    # searches: [(fx, dg, dg_init)]; with the switch off dg_init is not returned (NaN) and grad.d came with the product
    for k, prod in ((3, 1), (7, 5), (9, 8)):
        for (f1, g1, i1), (f0, g0, i0) in zip(lon[k], loff[k]):
            assert (f1, g1) == (f0, g0) and np.isnan(i0)
        assert lon[k][0][2] == loff[prod][1] < 0        # the grad.d of the full product, bit for bit
    assert np.isnan(lon[9][1][2])                       # a second trial returns none


def test_ascent_direction_is_refused_as_before(A, monkeypatch):
    """drt = +H grad from some iteration on: the search that follows throws the reference's message.  With the form on the
    entry check runs behind the pass of the first trial, which must not show: same text, same nfev, x as the search found it."""
    n, m = 4098, 3
    x0 = O.rosen_x0(n, 7)
    seen = {}

    def flip(k, s):
        if k == 4:
            s.set_direction_scale(1.0)

    for sw in ("1", "0"):
        seen[sw] = _run(A, monkeypatch, sw, A.ExtendedRosenbrock(), x0, O.F64, m, 12, A.LS_MORE_THUENTE, at_iteration=flip)
    on, off = seen["1"], seen["0"]
    print("ascent:", on["error"], on["nfev"], off["nfev"], on["last"], len(on["per_iter"]))
    assert on["error"] is not None and "the moving direction does not decrease the objective function value" in on["error"]
    assert on["error"] == off["error"] and on["nfev"] == off["nfev"] and len(on["per_iter"]) == len(off["per_iter"])
    assert np.array_equal(on["x"], off["x"]) and np.array_equal(on["g"], off["g"]) and np.array_equal(on["d"], off["d"])
    assert not np.array_equal(on["x"], x0)
    # the throwing search took grad.d from its first trial: one more step run by a trial than the iteration before it had seen
    assert on["before_download"][1] == on["per_iter"][-1][0][1] + 1
