"""-m gpu: the two-loop recursion d = a H v (BFGSMat.h:276-302) in every form the library has, against the exact reference
of tests/twoloop_ref.py (proved on the CPU by tests/test_twoloop_ref_cpu.py): ALL n elements of d, each of the 2c+1 dots
(lbfgsx_bfgs_download_dots) and the returned v.d, bit for bit.

  step launches        k_twoloop<TL_INIT | TL_SUB | TL_SUBDIV | TL_ADD> (LBFGSX_PERSIST=0): vector / tail boundary, tile
                       boundaries, both traversal directions, a grid that takes its stride twice, every history length
  persistent launch    k_twoloop_persist under both forms of the meeting points: the first and second register slot, the last
                       register and the first LDS slot, the streamed part with a partial tile and a scalar tail
  fused post form      lbfgsx_post_linesearch_spec: s, y, the four sums, the verdict, ys, theta, then the direction
  from the gradient    after an accepted post-form first trial, and the deferred last step run by k_trial_last, by
                       k_trial_settle and by k_twoloop<TL_ADD> ahead of another reader of D

Bit-for-bit comparison needs every exact sum of a case to lie further from a rounding boundary than the accumulators' error
bound; every test asserts that on the reference it uses and fails -- it does not skip -- where it does not hold.  The CPU
references of the large cases take 10 .. 30 s each; each is computed once (twoloop_ref caches them) and shared by the forms."""
import ctypes as C
import time

import numpy as np
import pytest

import statement_ref as R
import twoloop_ref as T

pytestmark = pytest.mark.gpu

CODE = {np.float64: 0, np.float32: 1}     # LBFGSX_F64, LBFGSX_F32
OBJ_QUAD = 0
REF_SECONDS = [0.0]                        # CPU time this file has spent in its references


def _timed(f, *args):
    t = time.perf_counter()
    out = f(*args)
    REF_SECONDS[0] += time.perf_counter() - t
    return out


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    core.lbfgsx_persistent_launches.restype = C.c_int64
    core.lbfgsx_persistent_launches.argtypes = [C.c_void_p]
    core.lbfgsx_persistent_resident_elems.restype = C.c_int64
    core.lbfgsx_persistent_resident_elems.argtypes = [C.c_void_p]
    core.lbfgsx_bfgs_stage_correction_host.restype = C.c_int
    core.lbfgsx_bfgs_stage_correction_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                       C.POINTER(C.c_double)]
    return A


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ctx:
    def __init__(self, A, dt, n, m):
        from lbfgspp_amd import _lib as L
        self.L, (self.core, _) = L, A.load()
        self.h = C.c_void_p()
        L.check(self.core.lbfgsx_create(C.byref(self.h), CODE[dt], n, m, 0, 0))
        self.n, self.m, self.dt = n, m, dt

    def up(self, which, arr):
        arr = np.ascontiguousarray(arr, self.dt)
        assert arr.shape == (self.n,)
        self.L.check(self.core.lbfgsx_upload(self.h, which, _p(arr)))

    def down(self, which):
        out = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, _p(out)))
        return out

    def add(self, s, y):
        s, y = np.ascontiguousarray(s, self.dt), np.ascontiguousarray(y, self.dt)
        self.L.check(self.core.lbfgsx_bfgs_add_correction_host(self.h, _p(s), _p(y)))

    def theta(self):
        return float(self.core.lbfgsx_bfgs_theta(self.h))

    def history(self):
        c = self.core.lbfgsx_bfgs_ncorr(self.h)
        S, Y = np.empty((max(c, 1), self.n), self.dt), np.empty((max(c, 1), self.n), self.dt)
        nc, ptr, th = C.c_int(), C.c_int(), C.c_double()
        self.L.check(self.core.lbfgsx_bfgs_download_history(self.h, _p(S), _p(Y), C.byref(nc), C.byref(ptr), C.byref(th)))
        assert nc.value == c
        return S[:c], Y[:c], ptr.value, th.value

    def dots(self, count):
        out = (C.c_double * count)()
        self.L.check(self.core.lbfgsx_bfgs_download_dots(self.h, out, count))
        return [float(v) for v in out]

    def apply(self, which, a):
        dg = C.c_double()
        self.L.check(self.core.lbfgsx_apply_Hv(self.h, which, float(a), C.byref(dg)))
        return dg.value

    def persist_counts(self):
        out = (C.c_int64 * 4)()
        self.L.check(self.core.lbfgsx_persist_counts(self.h, C.byref(out)))
        return tuple(int(v) for v in out)

    def counts(self, name, k):
        out = (C.c_int64 * k)()
        self.L.check(getattr(self.core, name)(self.h, C.byref(out)))
        return tuple(int(v) for v in out)

    def close(self):
        self.core.lbfgsx_destroy(self.h)


def _same_bits(got, want, what):
    """every element, and the sign of a zero"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want) or not np.array_equal(np.signbit(got), np.signbit(want)):
        bad = np.flatnonzero((got != want) | (np.signbit(got) != np.signbit(want)))
        raise AssertionError("%s: %d of %d elements differ, first at %d (got %r, reference %r), last at %d" % (
            what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], bad[-1]))


def _values(dots):
    return [float(d.value) for d in dots]


def _not_ambiguous(dots, what):
    for k, d in enumerate(dots):
        assert not d.ambiguous, "%s: exact sum %d lies within %.3g double ulp of a rounding boundary: choose another seed" % (
            what, k, float(d.bound / R.ulp(d.exact, np.float64)))


def _upload_history(c, cs, bt, S, Y, ptr, ref):
    """lbfgsx_bfgs_add_correction_host pair by pair, theta after every pair where the rows are few enough to afford the exact
    dots of the pairs that leave the ring again; then the history read back and held to the reference's"""
    for s, y in bt.pairs:
        c.add(s, y)
        if cs.n <= 70000:
            assert c.theta() == float(_timed(T.pair_scalars, s, y, cs.dtype)[1]), "theta after add_correction"
    k = min(cs.npairs, cs.m)
    assert c.core.lbfgsx_bfgs_ncorr(c.h) == k
    gS, gY, gptr, gtheta = c.history()
    assert gptr == ptr and gtheta == float(ref.theta) == c.theta()
    if k:
        _same_bits(gS, S, "S as stored")
        _same_bits(gY, Y, "Y as stored")


def _product(c, cs, bt, ref, products, what):
    """v (and, for the "other" inputs, a gradient that is not v) uploaded, `products` products in a row: D, the dots and the
    returned dot bit for bit every time"""
    L = c.L
    k = min(cs.npairs, cs.m)
    want_dots = _values(ref.dots)
    want_dg = ref.dg
    which = L.VEC_G
    if bt.g is not None:
        # v is not the gradient: both forms return v . d (include/lbfgsx.h), not G . d
        c.up(L.VEC_G, bt.g)
        which = L.VEC_GP
        last = _timed(T.rdot, bt.v, ref.d, cs.dtype)
        _not_ambiguous([last], what)
        assert float(last.value) != ref.dg          # G . d is another number: the two are told apart
        want_dots = want_dots[:-1] + [float(last.value)]
        want_dg = float(last.value)
    c.up(which, bt.v)
    for rep in range(products):
        dg = c.apply(which, bt.a)
        d = c.down(L.VEC_D)
        _same_bits(d, ref.d, "%s: D of product %d" % (what, rep))
        assert c.dots(2 * k + 1) == want_dots, "%s: dots of product %d" % (what, rep)
        assert dg == want_dg, "%s: returned dot of product %d" % (what, rep)


def _run_case(A, cs, products):
    bt = T.built(cs)
    S, Y, ptr, ref = _timed(T.reference, cs)
    _not_ambiguous(ref.dots, T.case_id(cs))
    c = Ctx(A, cs.dtype, cs.n, cs.m)
    try:
        _upload_history(c, cs, bt, S, Y, ptr, ref)
        _product(c, cs, bt, ref, products, T.case_id(cs))
        return c.persist_counts(), int(c.core.lbfgsx_persistent_launches(c.h))
    finally:
        c.close()


@pytest.fixture(scope="module")
def gth(A):
    """persist_grid * 256, read off a probing context: what lbfgsx_persistent_resident_elems caps at, over 45 slots of W"""
    n = 46 * T.GTH * 2
    c = Ctx(A, np.float64, n, 1)
    res = int(c.core.lbfgsx_persistent_resident_elems(c.h))
    c.close()
    assert res % ((T.NR + T.NL) * 2) == 0 and res < n
    got = res // ((T.NR + T.NL) * 2)
    assert got == T.GTH, "this device runs the persistent launch with %d threads; the sizes of twoloop_ref are built for %d" % (got, T.GTH)
    return got


# ---------------------------------------------------------------- the step launches
@pytest.mark.parametrize("cs", T.STEP_CASES, ids=T.case_id)
def test_step_launches(A, monkeypatch, cs):
    monkeypatch.setenv("LBFGSX_PERSIST", "0")
    products = 2 if cs in T.STEP_REV else 1      # 2c+1 launches each: the second product walks every step the other way
    counts, launches = _run_case(A, cs, products)
    assert launches == 0 and counts == (0, 0, 0, products)


@pytest.mark.parametrize("cs", T.STEP_M129, ids=T.case_id)
def test_step_launches_take_over_past_128_pairs(A, monkeypatch, cs):
    """m = 129 with the persistent form enabled: the column list of a persistent launch holds 128 pairs"""
    monkeypatch.setenv("LBFGSX_PERSIST", "1")
    monkeypatch.setenv("LBFGSX_PERSIST_MIN_N", "0")
    counts, launches = _run_case(A, cs, 1)
    assert launches == 0 and counts == (0, 0, 0, 1)


# ---------------------------------------------------------------- the persistent launch
def _persistent(monkeypatch, meet):
    monkeypatch.setenv("LBFGSX_PERSIST", "1")
    monkeypatch.setenv("LBFGSX_PERSIST_MIN_N", "0")
    monkeypatch.setenv("LBFGSX_MEET", meet)


@pytest.mark.parametrize("meet", ["all", "last"])
@pytest.mark.parametrize("cs", T.PERSIST_CASES, ids=T.case_id)
def test_persistent_launch(A, monkeypatch, gth, cs, meet):
    _persistent(monkeypatch, meet)
    counts, launches = _run_case(A, cs, 1)
    assert launches == 1 and counts == (1, 0, 0, 0)     # one persistent launch, no time-out, no step launches


@pytest.mark.parametrize("meet", ["all", "last"])
@pytest.mark.parametrize("cs", T.LARGE_CASES, ids=T.case_id)
def test_persistent_launch_slot_classes(A, monkeypatch, gth, cs, meet):
    """registers -> LDS at (30 gth +- 1) W + 1; LDS -> streamed part at (45 gth + 2 tiles + 37) W + (W - 1), which runs twice in
    a row so that the streamed tiles are walked in both directions against one reference"""
    _persistent(monkeypatch, meet)
    products = 2 if cs in T.LARGE_STREAM else 1
    W = T.width(cs.dtype)
    assert (cs.n // W > (T.NR + T.NL) * gth) == (cs in T.LARGE_STREAM) and cs.n // W > (T.NR - 1) * gth
    counts, launches = _run_case(A, cs, products)
    assert launches == products and counts == (products, 0, 0, 0)


# ---------------------------------------------------------------- ys of a pair
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_staged_pair_scalars(A, dt):
    """s.y and y.y as lbfgsx_bfgs_stage_correction_host returns them (the device keeps T(s.y) as the pair's ys), theta after
    the commit: the reference's bits"""
    cs = T.Case("hist", 3 * T.TILE * T.width(dt) + 300 * T.width(dt) + (T.width(dt) - 1), 3, 2, dt, 1)
    bt = T.built(cs)
    c = Ctx(A, dt, cs.n, cs.m)
    try:
        for s, y in bt.pairs:
            ys, theta, sy, yy = _timed(T.pair_scalars, s, y, dt)
            _not_ambiguous([sy, yy], "pair scalars")
            r = [C.c_double(), C.c_double()]
            c.L.check(c.core.lbfgsx_bfgs_stage_correction_host(c.h, _p(s), _p(y), C.byref(r[0]), C.byref(r[1])))
            assert (r[0].value, r[1].value) == (float(sy.value), float(yy.value))
            c.L.check(c.core.lbfgsx_commit_correction(c.h))
            assert c.theta() == float(theta)
    finally:
        c.close()


# ---------------------------------------------------------------- the inspection entry
def test_download_dots_reads_and_validates(A, monkeypatch):
    monkeypatch.setenv("LBFGSX_PERSIST", "0")
    cs = T.HISTORY[2]
    bt = T.built(cs)
    S, Y, ptr, ref = _timed(T.reference, cs)
    c = Ctx(A, cs.dtype, cs.n, cs.m)
    try:
        for s, y in bt.pairs:
            c.add(s, y)
        c.up(c.L.VEC_G, bt.v)
        c.apply(c.L.VEC_G, bt.a)
        want = _values(ref.dots)
        assert c.dots(len(want)) == want and c.dots(2) == want[:2] and c.dots(len(want)) == want   # reading changes nothing
        out = (C.c_double * 64)()
        E_INVALID = c.L.E_INVALID
        assert c.core.lbfgsx_bfgs_download_dots(c.h, out, 0) == E_INVALID
        assert c.core.lbfgsx_bfgs_download_dots(c.h, out, 2 * cs.m + 2) == E_INVALID
        assert c.core.lbfgsx_bfgs_download_dots(c.h, None, 1) == E_INVALID
        assert c.core.lbfgsx_bfgs_download_dots(None, out, 1) == E_INVALID
        assert c.core.lbfgsx_bfgs_download_dots(c.h, out, 2 * cs.m + 1) == 0
        _same_bits(c.down(c.L.VEC_D), ref.d, "D after the reads")
    finally:
        c.close()


# ---------------------------------------------------------------- the fused post form
def _post_case(A, monkeypatch, cs):
    monkeypatch.setenv("LBFGSX_PERSIST", "1")
    monkeypatch.setenv("LBFGSX_PERSIST_MIN_N", "0")
    monkeypatch.setenv("LBFGSX_FUSE_POST", "1")
    bt = T.post_built(cs)
    S, Y, ptr, post = _timed(T.post_reference, cs)
    what = T.post_case_id(cs)
    _not_ambiguous(post.sums + post.two_loop.dots, what)
    assert post.accepted == cs.accept
    dt = cs.dtype
    c = Ctx(A, dt, cs.n, cs.m)
    L = c.L
    try:
        for s, y in bt.pairs:
            c.add(s, y)
        before = min(cs.npairs, cs.m)
        c.up(L.VEC_X, bt.xp)
        c.up(L.VEC_G, bt.gp)
        L.check(c.core.lbfgsx_ls_begin(c.h))
        c.up(L.VEC_XT, bt.x)
        c.up(L.VEC_GT, bt.g)
        L.check(c.core.lbfgsx_ls_end(c.h, 0))
        r = [C.c_double() for _ in range(4)]
        L.check(c.core.lbfgsx_post_linesearch_spec(c.h, -1.0, *[C.byref(v) for v in r]))
        got = [v.value for v in r]
        for k, name in enumerate(("g.g", "x.x", "s.y", "y.y")):
            assert R.adjacent(got[k], post.sums[k].exact, dt), "%s: %s = %r, exact %.20g" % (what, name, got[k], float(post.sums[k].exact))
        assert got[2] == float(post.ys)                                    # the pair's ys, bit for bit
        assert (dt(got[2]) > dt(np.finfo(dt).eps) * dt(got[3])) == cs.accept
        assert c.counts("lbfgsx_spec_counts", 3) == (1, 0, 0 if cs.accept else 1)
        if cs.accept:
            L.check(c.core.lbfgsx_commit_correction(c.h))
            assert c.theta() == float(post.theta)
        dg = c.apply(L.VEC_G, -1.0)
        d = c.down(L.VEC_D)
        tl = post.two_loop
        _same_bits(d, tl.d, what + ": D")
        assert c.dots(len(tl.dots)) == _values(tl.dots) and dg == tl.dg
        assert c.counts("lbfgsx_spec_counts", 3) == (1, 1 if cs.accept else 0, 0 if cs.accept else 1)
        assert c.core.lbfgsx_bfgs_ncorr(c.h) == post.ncorr == min(before + (1 if cs.accept else 0), cs.m)
        pc = c.persist_counts()
        assert pc == (1 if cs.accept else 2, 0, 0, 0)     # the fused launch; after a rejected pair, the product's own
        if not cs.accept:
            # s and y of a rejected pair stay in the spare column: committing it now (nothing else follows) brings them into reach
            L.check(c.core.lbfgsx_commit_correction(c.h))
            assert c.theta() == float(post.theta)
        gS, gY, gptr, _ = c.history()
        loc = ptr % cs.m
        _same_bits(gS[loc], post.s, what + ": stored s")
        _same_bits(gY[loc], post.y, what + ": stored y")
        if cs.accept:
            assert gptr == post.ptr
            _same_bits(gS, post.S, what + ": S")
            _same_bits(gY, post.Y, what + ": Y")
    finally:
        c.close()


@pytest.mark.parametrize("cs", T.POST_CASES, ids=T.post_case_id)
def test_fused_post_form(A, monkeypatch, cs):
    _post_case(A, monkeypatch, cs)


@pytest.mark.parametrize("cs", T.POST_LARGE, ids=T.post_case_id)
def test_fused_post_form_with_a_streamed_part(A, monkeypatch, gth, cs):
    assert cs.n // T.width(cs.dtype) > (T.NR + T.NL) * gth
    _post_case(A, monkeypatch, cs)


# ---------------------------------------------------------------- from the gradient, and the deferred last step
class Driver:
    """The driver's statements through the C ABI on the diagonal quadratic, every search with the trials it is told to run"""

    def __init__(self, A, monkeypatch, dt, n):
        for k, v in (("LBFGSX_PERSIST", "1"), ("LBFGSX_PERSIST_MIN_N", "0"), ("LBFGSX_FUSE_POST", "1"), ("LBFGSX_POST_IN_TRIAL", "1"),
                     ("LBFGSX_LAST_IN_TRIAL", "1")):
            monkeypatch.setenv(k, v)
        self.q = _timed(T.quad_reference, dt, n)
        for it in self.q.iters:
            _not_ambiguous(it.post.sums + it.post.two_loop.dots, "quadratic n = %d" % n)
        self.c = c = Ctx(A, dt, n, T.QUAD_M)
        self.L, self.core, self.h = c.L, c.core, c.h
        L = self.L
        for which, v in ((L.VEC_A, self.q.a), (L.VEC_B, self.q.b), (L.VEC_X, self.q.x0)):
            c.up(which, v)
        L.check(self.core.lbfgsx_last_in_trial_request(self.h, 1))
        r = [C.c_double() for _ in range(3)]
        L.check(self.core.lbfgsx_eval(self.h, OBJ_QUAD, *[C.byref(v) for v in r]))
        _same_bits(c.down(L.VEC_G), self.q.iters[0].gp, "gradient at x0")
        dg = c.apply(L.VEC_G, -1.0)
        assert dg == self.q.iters[0].dg
        _same_bits(c.down(L.VEC_D), self.q.iters[0].d, "first direction")

    def search(self, steps):
        """[(fx, dg, dg_init)] of the trials; the search keeps the last one"""
        L, core, h = self.L, self.core, self.h
        L.check(core.lbfgsx_ls_begin(h))
        L.check(core.lbfgsx_ls_post_in_trial(h, -1.0))
        out = []
        for t in steps:
            fx, dgt, dg0 = C.c_double(), C.c_double(), C.c_double()
            L.check(core.lbfgsx_trial_first(h, OBJ_QUAD, float(t), C.byref(fx), C.byref(dgt), C.byref(dg0)))
            out.append((fx.value, dgt.value, dg0.value))
        return out

    def end(self):
        self.L.check(self.core.lbfgsx_ls_end(self.h, 0))

    def product(self, it):
        """the statements after the search that ended at it.x: the sums, the commit, the product; (pending, v.d)"""
        L, core, h = self.L, self.core, self.h
        r = [C.c_double() for _ in range(4)]
        L.check(core.lbfgsx_post_linesearch_spec(h, -1.0, *[C.byref(v) for v in r]))
        assert [v.value for v in r] == _values(it.post.sums)
        L.check(core.lbfgsx_commit_correction(h))
        assert self.c.theta() == float(it.post.theta)
        dg, pending = C.c_double(), C.c_int(0)
        L.check(core.lbfgsx_apply_Hv_pending(h, L.VEC_G, -1.0, C.byref(dg), C.byref(pending)))
        return pending.value, dg.value

    def last_counts(self):
        return self.c.counts("lbfgsx_last_in_trial_counts", 4)

    def to_the_pending_step(self):
        """two iterations: a plain first trial and the fused post form, then an accepted post-form first trial and the launch
        from the gradient, which ends one step early.  Returns the Iter whose post.two_loop is the product that is owed its last
        step."""
        it0, it1 = self.q.iters[0], self.q.iters[1]
        (_, _, dg0), = self.search([T.QUAD_STEPS[0]])
        self.end()
        assert np.isnan(dg0)
        pending, dg = self.product(it0)
        assert pending == 0 and dg == it0.post.two_loop.dg == it1.dg
        assert self.c.dots(3) == _values(it0.post.two_loop.dots)
        assert self.c.counts("lbfgsx_spec_counts", 3) == (1, 1, 0) and self.last_counts() == (0, 0, 0, 1)
        (_, _, dg0), = self.search([T.QUAD_STEPS[1]])
        self.end()
        assert np.isnan(dg0)
        pending, dg = self.product(it1)
        assert pending == 1 and np.isnan(dg)
        assert self.last_counts() == (1, 0, 0, 1)
        assert self.c.counts("lbfgsx_post_in_trial_counts", 4) == (1, 1, 1, 1)
        tl = it1.post.two_loop
        assert len(tl.dots) == 5 and self.c.dots(4) == _values(tl.dots)[:4]      # the launch ended with step 2c-1
        assert self.last_counts() == (1, 0, 0, 1)                                # reading them settled nothing
        assert self.c.persist_counts()[1] == 0
        return it1

    def close(self):
        self.c.close()


@pytest.mark.parametrize("dt,n", T.QUAD_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_last_step_run_by_the_first_trial(A, monkeypatch, gth, dt, n):
    """k_trial_last: dg_init is the reference's v.d, the trial point is xp + step d_ref (read once the search has accepted it
    and the next product has run, so that no step is settled for the download), the step's dot is in its slot"""
    dr = Driver(A, monkeypatch, dt, n)
    try:
        it1 = dr.to_the_pending_step()
        it2 = dr.q.iters[2]
        tl = it1.post.two_loop
        (_, _, dg0), = dr.search([T.QUAD_STEPS[2]])
        assert dg0 == tl.dg == it2.dg
        assert dr.last_counts() == (1, 1, 0, 1)
        assert dr.c.dots(5)[4] == tl.dg
        dr.end()
        pending, _ = dr.product(it2)
        assert pending == 1 and dr.last_counts() == (2, 1, 0, 1)
        assert dr.c.counts("lbfgsx_post_in_trial_counts", 4) == (2, 2, 2, 1)
        _same_bits(dr.c.down(dr.L.VEC_X), it2.x, "trial point")          # = R.axpy_ref(xp, d_ref, step)
        assert dr.last_counts() == (2, 1, 1, 1)                          # the download ran the step the new product owed
        _same_bits(dr.c.down(dr.L.VEC_D), it2.post.two_loop.d, "next direction")
        assert dr.c.dots(7) == _values(it2.post.two_loop.dots)
    finally:
        dr.close()


@pytest.mark.parametrize("dt,n", T.QUAD_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_last_step_run_by_a_settling_trial(A, monkeypatch, gth, dt, n):
    """the first trial forms the step and is rejected by the caller; the second one (k_trial_settle) forms it again and stores D"""
    dr = Driver(A, monkeypatch, dt, n)
    try:
        it1 = dr.to_the_pending_step()
        it2 = dr.q.iters[2]
        tl = it1.post.two_loop
        second = 0.375
        (_, _, dg_a), (_, _, dg_b) = dr.search([T.QUAD_STEPS[2], second])
        assert dg_a == tl.dg and np.isnan(dg_b)
        assert dr.last_counts() == (1, 1, 1, 1)
        _same_bits(dr.c.down(dr.L.VEC_D), tl.d, "D as the settling trial stored it")
        _same_bits(dr.c.down(dr.L.VEC_XT), R.axpy_ref(it2.xp, tl.d, second), "trial point")
        assert dr.last_counts() == (1, 1, 1, 1)
    finally:
        dr.close()


@pytest.mark.parametrize("dt,n", T.QUAD_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_last_step_run_ahead_of_a_download(A, monkeypatch, gth, dt, n):
    """lbfgsx_download(VEC_D) runs k_twoloop<TL_ADD> first; the first trial that follows is a plain post-form one and hands out
    the v.d the step left in its slot"""
    dr = Driver(A, monkeypatch, dt, n)
    try:
        it1 = dr.to_the_pending_step()
        it2 = dr.q.iters[2]
        tl = it1.post.two_loop
        _same_bits(dr.c.down(dr.L.VEC_D), tl.d, "D after the step launch")
        assert dr.last_counts() == (1, 0, 1, 1)
        assert dr.c.dots(5) == _values(tl.dots)
        (_, _, dg0), = dr.search([T.QUAD_STEPS[2]])
        assert dg0 == tl.dg
        _same_bits(dr.c.down(dr.L.VEC_XT), it2.x, "trial point")
        assert dr.last_counts() == (1, 0, 1, 1)
    finally:
        dr.close()


def test_zz_reference_time():
    """not a check of the library: prints what the references of this file have cost on the CPU (run the file as a whole)"""
    print("twoloop references: %.1f s of CPU time" % REF_SECONDS[0])
