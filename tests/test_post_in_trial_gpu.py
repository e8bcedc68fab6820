"""GPU suite: the post form of the first trial (k_trial_post, lbfgsx_ls_post_in_trial) and the persistent launch that starts
the recursion from the gradient (PersistArgs::from_g).

The trial's pass forms s, y, the four post sums and the recursion's first dot with the expressions of step 0 of the fused
launch, so every run with the form on (the default) is compared bit for bit -- np.array_equal -- with the same run under
LBFGSX_POST_IN_TRIAL=0: x, grad, the direction and the whole history (its newest pair is what the spare column received)
after every iteration, and niter, nfev, fx at the end.  The shapes are the smallest at which each code path exists."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle_lib as O
from test_term_objective_cpu import ROSEN

pytestmark = pytest.mark.gpu

# elements of q a persistent launch keeps on the CUs of an MI355X: 45 slots x 512 blocks x 256 threads x 16 bytes
RESIDENT = {O.F64: 11_796_480, O.F32: 23_592_960}


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


def _counts(core, h):
    """{post-form trials issued, accepted, launches that started from the gradient, form enabled}"""
    out = (C.c_int64 * 4)()
    assert core.lbfgsx_post_in_trial_counts(h, C.byref(out)) == 0
    return tuple(int(v) for v in out)


def _persist(core, h):
    out = (C.c_int64 * 4)()
    core.lbfgsx_persist_counts(h, C.byref(out))
    return tuple(int(v) for v in out)


def _down(core, L, h, which, n, dt):
    out = np.empty(n, dt)
    L.check(core.lbfgsx_download(h, which, out.ctypes.data_as(C.c_void_p)))
    return out


def _history(core, L, h, n, m, dt):
    nc = core.lbfgsx_bfgs_ncorr(h)
    S, Y = np.zeros((max(nc, 1), n), dt), np.zeros((max(nc, 1), n), dt)
    ncorr, ptr, theta = C.c_int(), C.c_int(), C.c_double()
    L.check(core.lbfgsx_bfgs_download_history(h, S.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), C.byref(ncorr),
                                              C.byref(ptr), C.byref(theta)))
    return S[:nc], Y[:nc], (ncorr.value, ptr.value, theta.value)


def _run(A, monkeypatch, switch, f, x0, dtype, m, iters, ls, history_every_iteration=True):
    """one solve; what it leaves after every iteration and at its end"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    core.lbfgsx_persistent_resident_elems.restype = C.c_int64
    core.lbfgsx_persistent_resident_elems.argtypes = [C.c_void_p]
    monkeypatch.setenv("LBFGSX_POST_IN_TRIAL", switch)
    gc.collect()
    dt, n = O.NPDT[dtype], x0.size
    s = A.LBFGSSolver(A.LBFGSParam(m=m, epsilon=0.0, epsilon_rel=0.0, max_iterations=iters), linesearch=ls, dtype=dt)
    tr = A.TraceBuffer(n, cap=512, with_x=False)
    per_iter = []

    def hook(k):
        h = s.ctx
        rec = [_down(core, L, h, w, n, dt) for w in (L.VEC_X, L.VEC_G, L.VEC_D)]
        if history_every_iteration:
            S, Y, meta = _history(core, L, h, n, m, dt)
            rec += [S, Y, np.array(meta)]
        per_iter.append((rec, tr.count, _counts(core, h)))

    s.set_iteration_hook(hook)
    x = x0.copy()
    niter, fx = s.minimize(f, x, trace=tr)
    h = s.ctx
    S, Y, meta = _history(core, L, h, n, m, dt)
    out = dict(niter=niter, nfev=s.last.nfev, fx=fx, x=x, fxs=tr.fx[:tr.count].copy(), per_iter=per_iter, S=S, Y=Y, meta=meta,
               counts=_counts(core, h), persist=_persist(core, h),
               resident=int(core.lbfgsx_persistent_resident_elems(h)))
    s.close()
    del s
    gc.collect()
    return out


def _same_bits(on, off):
    assert (on["niter"], on["nfev"]) == (off["niter"], off["nfev"]) and on["fx"] == off["fx"]
    assert np.array_equal(on["x"], off["x"]) and np.array_equal(on["fxs"], off["fxs"])
    assert len(on["per_iter"]) == len(off["per_iter"]) > 0
    for k, ((ra, ca, _), (rb, cb, _)) in enumerate(zip(on["per_iter"], off["per_iter"])):
        assert ca == cb, "evaluations up to iteration %d" % (k + 1)
        for a, b in zip(ra, rb):
            assert np.array_equal(a, b), "iteration %d" % (k + 1)
    assert np.array_equal(on["S"], off["S"]) and np.array_equal(on["Y"], off["Y"]) and on["meta"] == off["meta"]
    assert off["counts"] == (0, 0, 0, 0)


def _quad(A, n, dtype):
    a, b = O.quad_problem(n, 10.0, 1, dtype)
    return A.DiagQuadratic(a, b), np.zeros(n, O.NPDT[dtype])


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("n,m", [(4096, 5), (4099, 5), (4099, 1), (4099, 40)])
def test_resident_only(A, monkeypatch, dtype, n, m):
    """q fits on the CUs: step 0 of the launch from the gradient fills the resident slots and nothing else.  n = 4099 has a
    scalar tail; m = 1 is the shortest recursion (steps 1 and 2 only), m = 40 a history longer than the run."""
    f, x0 = _quad(A, n, dtype)
    on, off = (_run(A, monkeypatch, sw, f, x0, dtype, m, 12, A.LS_NOCEDAL_WRIGHT) for sw in ("1", "0"))
    _same_bits(on, off)
    issued, accepted, from_g, enabled = on["counts"]
    assert enabled == 1 and accepted >= 5 and from_g == accepted and issued >= accepted
    assert on["persist"][1] == 0 and on["persist"][3] == 0   # no time-out, no product by step launches


@pytest.mark.parametrize("dtype,obj,k", [(O.F64, "quad", 3), (O.F32, "quad", 3), (O.F64, "rosen", 5)])
def test_streamed_step_1_reads_the_gradient(A, monkeypatch, dtype, obj, k):
    """One element (Rosenbrock: one pair) and a few tiles past the resident capacity: step 1 of the launch forms a*g from g
    for the streamed tiles and the scalar tail.  The quadratic accepts every first trial (one traversal parity); the
    Rosenbrock run likewise from its second search on (17 trials in the first)."""
    n = RESIDENT[dtype] + 1024 * k + (1 if obj == "quad" else 2)
    if obj == "quad":
        f, x0 = _quad(A, n, dtype)
        ls, iters = A.LS_NOCEDAL_WRIGHT, 6
    else:
        f, x0, ls, iters = A.ExtendedRosenbrock(), O.rosen_x0(n, 7, dtype), A.LS_MORE_THUENTE, 9
    on, off = (_run(A, monkeypatch, sw, f, x0, dtype, 3, iters, ls, history_every_iteration=False) for sw in ("1", "0"))
    _same_bits(on, off)
    assert on["resident"] == RESIDENT[dtype] < n
    issued, accepted, from_g, _ = on["counts"]
    assert accepted >= 2 and from_g == accepted
    assert on["persist"][1] == 0 and on["persist"][3] == 0
    # The traversal direction of step L of a persistent launch is the parity of (launches issued before it + L): every
    # trial counts one, a product on c pairs 2c + 1 (the first, on the empty history, one).  All pairs of these runs are
    # accepted, so search k is followed by a product on min(k, m) pairs, and the parity of a launch follows from the
    # evaluations per search recorded by the hook.
    evals = np.diff([1] + [c for _, c, _ in on["per_iter"]])
    fg = np.diff([0] + [c[2] for _, _, c in on["per_iter"]])
    issued_before, parities = 1, set()
    for k in range(len(evals)):
        issued_before += int(evals[k])
        if fg[k]:
            parities.add((issued_before + 1) & 1)          # step 1, the first streamed step of a launch from the gradient
        issued_before += 2 * min(k + 1, 3) + 1
    assert on["meta"][0] == 3                                # the history filled up: every pair was accepted
    # after the first search every search of these runs accepts its first trial, so their launches keep one direction (the
    # other one: test_streamed_step_1_in_both_traversal_directions)
    assert len(parities) == 1, (evals.tolist(), fg.tolist(), parities)


def test_step_launches_below_the_persistent_threshold(A, monkeypatch):
    """n = 2047 with the product's threshold (4096): the products are 2c+1 step launches, whose first launch forms a*g and
    its dot again -- the same sum the trial left."""
    monkeypatch.setenv("LBFGSX_PERSIST_MIN_N", "4096")
    f, x0 = _quad(A, 2047, O.F64)
    on, off = (_run(A, monkeypatch, sw, f, x0, O.F64, 4, 12, A.LS_NOCEDAL_WRIGHT) for sw in ("1", "0"))
    _same_bits(on, off)
    issued, accepted, from_g, _ = on["counts"]
    assert accepted >= 5 and from_g == 0 and on["persist"][0] == 0 and on["persist"][3] > 0


def test_rejected_first_trials_fall_back_to_the_plain_form(A, monkeypatch):
    """Rosenbrock from the benchmark's start point, first 12 iterations: some searches reject their first trial.  Both
    branches occur, a search after a rejection starts with a plain trial, and a search after a first-trial acceptance
    (with a non-empty history) starts with the post form."""
    n = 300_002
    on, off = (_run(A, monkeypatch, sw, A.ExtendedRosenbrock(), O.rosen_x0(n, 7), O.F64, 10, 12, A.LS_MORE_THUENTE)
               for sw in ("1", "0"))
    _same_bits(on, off)
    issued, accepted, from_g, _ = on["counts"]
    assert accepted >= 1 and issued > accepted and from_g == accepted
    evals = np.diff([1] + [c for _, c, _ in on["per_iter"]])        # trials of search k (the first evaluation is at x0)
    iss = np.diff([0] + [c[0] for _, _, c in on["per_iter"]])       # post-form trials issued in search k
    assert iss[0] == 0                                              # empty history
    for k in range(1, len(evals)):
        assert iss[k] == (1 if evals[k - 1] == 1 else 0), (k, evals.tolist(), iss.tolist())


def test_term_objective_same_bits_and_chain_objective_keeps_the_plain_form(A, monkeypatch):
    """A TermObjective restatement of Rosenbrock gives the bits of the built-in objective with the form on; a context bound
    to a chain objective never asks for the post form."""
    n = 4096 + 2
    x0 = O.rosen_x0(n, 7)
    builtin = _run(A, monkeypatch, "1", A.ExtendedRosenbrock(), x0, O.F64, 6, 14, A.LS_MORE_THUENTE)
    term = _run(A, monkeypatch, "1", A.TermObjective(ROSEN, K=2), x0, O.F64, 6, 14, A.LS_MORE_THUENTE)
    off = _run(A, monkeypatch, "0", A.TermObjective(ROSEN, K=2), x0, O.F64, 6, 14, A.LS_MORE_THUENTE)
    _same_bits(term, off)
    _same_bits(builtin, off)
    assert builtin["counts"][1] >= 1 and builtin["counts"][2] == builtin["counts"][1]
    assert term["counts"][1] >= 1 and term["counts"] == builtin["counts"]   # the compiled kernels have the post form too
    chain = A.ChainObjective("const T d = x[1] - x[0];\ng[0] = -d + x[0];\ng[1] = d;\nreturn T(0.5) * (d * d + x[0] * x[0]);", K=2)
    c = _run(A, monkeypatch, "1", chain, np.linspace(-1.0, 1.0, n), O.F64, 6, 10, A.LS_NOCEDAL_WRIGHT)
    assert c["counts"][:3] == (0, 0, 0)


class _Manual:
    """The driver's statements through the C ABI, one search = one trial at a given step (no Wolfe test): what lets a test
    interleave two contexts and choose the points."""

    def __init__(self, A, monkeypatch, switch, n, m, a, b, x0):
        from lbfgspp_amd import _lib as L
        self.L, (self.core, _) = L, A.load()
        monkeypatch.setenv("LBFGSX_POST_IN_TRIAL", switch)
        self.h = C.c_void_p()
        L.check(self.core.lbfgsx_create(C.byref(self.h), O.F64, n, m, 0, 0))
        self.n = n
        for which, v in ((L.VEC_A, a), (L.VEC_B, b), (L.VEC_X, x0)):
            L.check(self.core.lbfgsx_upload(self.h, which, np.ascontiguousarray(v, np.float64).ctypes.data_as(C.c_void_p)))
        r = [C.c_double() for _ in range(3)]
        L.check(self.core.lbfgsx_eval(self.h, O.OBJ_QUAD, *[C.byref(v) for v in r]))
        dg = C.c_double()
        L.check(self.core.lbfgsx_apply_Hv(self.h, L.VEC_G, -1.0, C.byref(dg)))

    def iteration(self, step, rejected_first=None, history=True):
        """one search and what follows it; rejected_first: a first trial at that step which the search does not keep"""
        L, core, h = self.L, self.core, self.h
        L.check(core.lbfgsx_ls_begin(h))
        L.check(core.lbfgsx_ls_post_in_trial(h, -1.0))
        fx, dgt = C.c_double(), C.c_double()
        if rejected_first is not None:
            L.check(core.lbfgsx_trial(h, O.OBJ_QUAD, rejected_first, C.byref(fx), C.byref(dgt)))
        L.check(core.lbfgsx_trial(h, O.OBJ_QUAD, step, C.byref(fx), C.byref(dgt)))
        L.check(core.lbfgsx_ls_end(h, 0))
        r = [C.c_double() for _ in range(4)]
        L.check(core.lbfgsx_post_linesearch_spec(h, -1.0, *[C.byref(v) for v in r]))
        g2, x2, sy, yy = [v.value for v in r]
        accepted = sy > np.finfo(np.float64).eps * yy
        if accepted:
            L.check(core.lbfgsx_commit_correction(h))
        dg = C.c_double()
        L.check(core.lbfgsx_apply_Hv(h, L.VEC_G, -1.0, C.byref(dg)))
        vec = [_down(core, L, h, w, self.n, np.float64) for w in (L.VEC_X, L.VEC_G, L.VEC_D)]
        S, Y, meta = _history(core, L, h, self.n, 0, np.float64) if history else (np.zeros(0), np.zeros(0), ())
        return dict(scalars=(fx.value, dgt.value, g2, x2, sy, yy, dg.value), accepted=accepted, vec=vec + [S, Y], meta=meta)

    def counts(self):
        return _counts(self.core, self.h)

    def close(self):
        self.core.lbfgsx_destroy(self.h)


def _same_iteration(a, b):
    assert a["scalars"] == b["scalars"] and a["accepted"] == b["accepted"] and a["meta"] == b["meta"]
    for u, v in zip(a["vec"], b["vec"]):
        assert np.array_equal(u, v)


def test_pair_rejected_by_the_curvature_test(A, monkeypatch):
    """s.y <= eps y.y (LBFGS.h:161), the case of test_fused_post_launch_statement_level, produced by the trial kernel itself:
    the quadratic with a = 1e9 has y = a^2 s, so s.y / y.y = 1e-18 < eps.  The post-form trial is accepted by the search,
    the host sees the pair fail the test, nothing is committed and the direction is computed the ordinary way on the old
    history.  The pair the spare column received is read back by committing it afterwards."""
    n, m = 4099, 4
    rng = np.random.default_rng(3)
    a_ok, b = np.linspace(1.0, 3.0, n), rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    res = {}
    for sw in ("1", "0"):
        c = _Manual(A, monkeypatch, sw, n, m, a_ok, b, x0)
        its = [c.iteration(1.0) for _ in range(3)]     # builds a history; from the second on the post form is in use
        before = c.counts()
        L = c.L
        L.check(c.core.lbfgsx_upload(c.h, L.VEC_A, np.full(n, 1e9).ctypes.data_as(C.c_void_p)))
        its.append(c.iteration(1e-12))                 # g at the trial point comes from a = 1e9: the pair is rejected
        assert not its[-1]["accepted"]
        after = c.counts()
        L.check(c.core.lbfgsx_commit_correction(c.h))  # the rejected pair is still pending in the spare column
        S, Y, meta = _history(c.core, L, c.h, n, m, np.float64)
        res[sw] = (its, S, Y, meta, before, after)
        c.close()
    for x, y in zip(res["1"][0], res["0"][0]):
        _same_iteration(x, y)
    assert np.array_equal(res["1"][1], res["0"][1]) and np.array_equal(res["1"][2], res["0"][2]) and res["1"][3] == res["0"][3]
    before, after = res["1"][4], res["1"][5]
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[2] == before[2]   # accepted trial, no launch from g
    assert res["0"][5] == (0, 0, 0, 0)


def test_streamed_step_1_in_both_traversal_directions(A, monkeypatch):
    """The streamed size again, driven statement by statement so that one search takes two trials: its post-form first
    trial is rejected (the fused launch that follows overwrites the spare column), the next search starts plain, and the
    launches from the gradient after it walk the tiles of step 1 in the other direction -- an even number of trials flips
    the parity of everything behind it.  The direction of step L of a persistent launch is the parity of (launches issued
    before it + L): one per trial, 2c + 1 per product on c pairs, one for the first product on the empty history."""
    n, m = RESIDENT[O.F64] + 1024 * 3 + 1, 3
    a, b = O.quad_problem(n, 10.0, 1, O.F64)
    x0 = np.zeros(n)
    trials = [1, 1, 1, 2, 1, 1, 1]
    res = {}
    for sw in ("1", "0"):
        c = _Manual(A, monkeypatch, sw, n, m, a, b, x0)
        its, fg = [], []
        for k, t in enumerate(trials):
            before = c.counts()[2]
            its.append(c.iteration(1.0, rejected_first=0.5 if t == 2 else None, history=k == len(trials) - 1))
            fg.append(c.counts()[2] - before)
            assert its[-1]["accepted"]
        res[sw] = (its, fg, c.counts())
        c.close()
    for x, y in zip(res["1"][0], res["0"][0]):
        _same_iteration(x, y)
    fg = res["1"][1]
    assert fg == [0, 1, 1, 0, 0, 1, 1] and res["1"][2][:3] == (5, 4, 4) and res["0"][2] == (0, 0, 0, 0)
    issued_before, parities = 1, []
    for k, t in enumerate(trials):
        issued_before += t
        if fg[k]:
            parities.append((issued_before + 1) & 1)
        issued_before += 2 * min(k + 1, m) + 1
    assert parities[:2] == [parities[0]] * 2 and parities[2:] == [1 - parities[0]] * 2, parities


def test_two_live_solvers_on_one_device(A, monkeypatch):
    """Two contexts on one device, driven alternately from one thread: both use the post form and the launch from the
    gradient, and each follows, bit for bit, the trajectory it has with the form off."""
    m = 3
    prob = []
    for n, seed in ((4099, 1), (6002, 2)):
        rng = np.random.default_rng(seed)
        prob.append((n, np.linspace(1.0, 2.0 + seed, n), rng.standard_normal(n), rng.standard_normal(n)))
    res = {}
    for sw in ("1", "0"):
        cs = [_Manual(A, monkeypatch, sw, n, m, a, b, x0) for n, a, b, x0 in prob]
        its = [[], []]
        for _ in range(6):
            for k, c in enumerate(cs):
                its[k].append(c.iteration(1.0))
        res[sw] = (its, [c.counts() for c in cs])
        for c in cs:
            c.close()
    for k in range(2):
        for x, y in zip(res["1"][0][k], res["0"][0][k]):
            _same_iteration(x, y)
        issued, accepted, from_g, _ = res["1"][1][k]
        assert issued == accepted == from_g == 5        # searches 2..6: the first has neither a history nor a precedent
        assert res["0"][1][k] == (0, 0, 0, 0)
