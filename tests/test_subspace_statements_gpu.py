"""-m gpu: the device side of the L-BFGS-B subspace minimisation (BOXCQP) against tests/subspace_ref.py, which
tests/test_subspace_ref_cpu.py proves against a scalar transcription of the reference and against the oracle.  The A/B tests
of test_lbfgsb_gpu.py compare one device form with another; all forms share sweep_row / sweep_row_v, the list append and
the reductions, so a wrong branch on a tie, a multiplier stored on the wrong row, a dropped tail row, a row lost from the
L u U list or a stale rhs passes them.  Here every vector and state byte is compared bit for bit over ALL n rows, every count
exactly, every sum with bounded_sums_ref.check_rounded / check_pair (dd_bound), the index list as a set.  No other tolerance.

Set-up through the ABI only: pairs with lbfgsx_bfgs_add_correction_host; x0, lb, ub and g per row (subspace_ref.build_rows:
some bounds infinite), lbfgsx_b_cauchy_build, lbfgsx_b_cauchy_finish(1, 1, 0), lbfgsx_b_sub_begin.  A row with lb == ub is
never free (its break point is 0, Cauchy.h:113), so the free rows with l == u have adjacent bounds and an x0 that is moved
1024 away after lbfgsx_b_sub_begin: lb - x0 and ub - x0 then round to the same number.
The state bytes, x0, lb, ub, g and drt are downloaded; the references use the downloaded values.  Before each call every
sub-vector is filled through lbfgsx_b_sub_upload: the statement's inputs on the free rows (subspace_ref.edge_values: y == l and
y == u with the multiplier > 0, +0, -0, < 0, l == u == y, one ulp inside and outside each bound, infinite bounds; a second
input moves every row to another class, so rows go L -> P, U -> P, P -> L, P -> U, L -> U between two sweeps), distinct finite
sentinels everywhere else.  After each call all six vectors, drt and the state bytes are downloaded and compared with the
reference, so a row outside the statement's mask must still hold its sentinel and a non-free state byte must be unchanged.
Finite inputs only: NaN handling is out of scope.

Found by this file (test_compact_sweeps): the pass that starts the compact vectors (k_solve_sweep / kx_solve_sweep, cv = 1) wrote
rhs by position only on the rows of the new P, and k_cv_back put the never-written positions of the rows of L and U back at
their rows -- whatever the buffer held replaced the row's rhs.  No statement reads rhs outside P before rewriting it, so no
result changed, but the by-row and the compact form were not the same bits; the pass now carries the row's rhs along.

Entry points, kernel classes and the shapes that reach them (csrc/lbfgsb_subspace.hip, lbfgsb_dots.hip, lbfgsb_x.hip):
  lbfgsx_b_sub_partition, _sub_check, _sub_sweep_begin (first = 1, 0), _sub_op x 6      test_partition_rows, test_all_or_none
      k_sub_partition / k_sub_check / k_sub_sweep_begin / k_sub_op, grid_for(n) = min(1024, ceil(n / W / 256)) blocks of 256,
      W = 2 (f64) or 4 (f32): n = 1, 2, 3, 63, 64, 65, 255, 256, 257, 256 W - 1, 256 W + 1 (the rows of one block), and
      1024 * 256 * W + 256 * W + 1 (every block walks a second stride).  The edge classes need >= 255 rows (asserted on the CPU);
      the smaller n test the geometry with the classes that fit.
  lbfgsx_b_wcombine x 5 modes                                                             test_wcombine
      k_wcombine<mode>, coef NULL and given, every selector for CB_SOLVE; masks inside L u U walk the index list when there
      is one (both routes run); c = 0, 1, 4, 5, 8, 10, 13, 20, 40 at n = 1501
  lbfgsx_b_solve_wty                                                                      test_solve_wty
      k_solve_dots<NC = 8, 16, 24, 32> (c = 1, 4 | 5, 8 | 10 | 13), min(512, grid_for) blocks; pmask = fmask = FREE and
      pmask = P inside fmask = FREE; c = 20 (2c > 32) must be refused; n = 1501 and 512 * 256 * 2 + 513 (c = 2)
  lbfgsx_b_solve_sweep (first = 1; first = 0 + lbfgsx_b_lu_sweep), _solve_sweep_rhs, _wtv_lu, _wtv_lu_c    test_fused_sweeps
      default: kx_solve_sweep<NCL, G> / kx_list2 / k_lu_sweep, (NCL, G) by 2c: c = 1, 4 (4, 2); 5 (6, 2); 8 (8, 2); 10 (10, 2);
      12 (12, 2); 13 (16, 2); 20 (20, 2); 24 (24, 2); 30 (30, 2); 40 (20, 4).  128 (G = 2) or 64 (G = 4) rows per block, one or
      two blocks per CU: n = 1501 is a dozen blocks with a tail; n = 70001 and 262657 (c <= 2) make every block stride.
      LBFGSX_SPLIT=0: k_solve_sweep<NC = 8, 16, 20, 24, 32> (c = 4, 8, 10, 12, 16), k_multidot_list2<8, 16, 24> (refused at
      c = 16: 2c > 24); c = 20 (NC > 32) refused.
      "tie" runs solve v / 1 without coefficients, so y lands on the bounds exactly and the ties of sweep_row_v are decided.
  lbfgsx_b_wtv_prologue, lbfgsx_b_gram_fused_ex with LBFGSX_GP_RHS                        test_gp_rhs
      kx_rows<NCL, G, 1> (k_vrows with LBFGSX_SPLIT=0) and the one-pass Gram's prologue, masks P and FREE
  refusals by value with the state unchanged                                              test_refusals
  the index list                                                                          test_lds_buffer, test_list_thresholds
      kListBuf = 1024: f32, all rows in L u U, n = 1024 * B (every block's buffer exactly full) and n above the grid cap
      (blocks 0..3 hold 1280 rows: the buffer and the direct append both contribute); kLuMax: |L u U| = 262144 / 262145 in the
      partition before; lu_cap = min(n, 2^20): |L u U| > 2^20 at n = 2^20 + 4096
  the compact copy and the compact vectors                                                test_compact_full_pass, test_compact_sweeps
      nfree = 4096, floor(7n / 8) (copy taken) and floor(7n / 8) + 1 (not taken); the sweep sequence on live compact vectors,
      with LBFGSX_COMPACT_VEC=0 and with a download in mid-sequence (k_cv_back<0>), all against one reference"""
import ctypes as C

import numpy as np
import pytest

import bounded_sums_ref as B
import subspace_ref as S

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double
pd = C.POINTER(f64)
E_INVALID = -1
THETA = 1.3


@pytest.fixture(scope="module")
def lib():
    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1
    pi64 = C.POINTER(i64)
    for name, args in (("lbfgsx_b_cauchy_build", [vp, pi64, pi64, pd, vp]),
                       ("lbfgsx_b_cauchy_finish", [vp, f64, f64, i32, pi64, pi64]),
                       ("lbfgsx_b_sub_begin", [vp]), ("lbfgsx_b_download_state", [vp, vp]),
                       ("lbfgsx_b_sub_partition", [vp, pi64, pi64, pi64]), ("lbfgsx_b_sub_check", [vp, vp]),
                       ("lbfgsx_b_sub_sweep_begin", [vp, i32, pi64, pi64, pi64, vp]), ("lbfgsx_b_sub_op", [vp, i32]),
                       ("lbfgsx_b_wcombine", [vp, i32, i32, i32, vp, f64]),
                       ("lbfgsx_b_solve_wty", [vp, i32, i32, vp, f64, i32, vp]),
                       ("lbfgsx_b_solve_sweep", [vp, i32, i32, vp, f64, vp, vp]),
                       ("lbfgsx_b_lu_sweep", [vp, vp, f64, vp]),
                       ("lbfgsx_b_wtv_lu", [vp, vp, pi64, vp, pi64]),
                       ("lbfgsx_b_wtv_prologue", [vp, i32, i32, i32, vp, vp, vp]),
                       ("lbfgsx_b_gram_fused_ex", [vp, i32, i32, i32, vp, vp, vp, vp]),
                       ("lbfgsx_b_gram_fused_dd", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                       ("lbfgsx_b_set_compaction", [vp, i32])):
        f = getattr(core, name)
        f.restype, f.argtypes = i32, args
    return core, L


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _pd(a):
    return None if a is None else a.ctypes.data_as(pd)


class Sub:
    """one bounded context brought to the start of a subspace minimisation; V mirrors the device vectors on the host"""

    def __init__(self, lib, n, c, dt, seed, m=None, nfree=None, free_all=False, finite_only=False):
        self.core, self.L = lib
        core, L = lib
        self.dt, self.n, self.c, self.t = np.dtype(dt).type, n, c, 2 * c
        self.h = vp()
        L.check(core.lbfgsx_create(C.byref(self.h), L.F64 if dt == F64 else L.F32, n, max(m or c, 1), 0, L.FLAG_BOUNDED))
        try:
            self.pairs, self.cols = S.history(n, c, dt, seed)
            for s_, y_ in self.pairs:
                L.check(core.lbfgsx_bfgs_add_correction_host(self.h, _p(s_), _p(y_)))
            assert core.lbfgsx_bfgs_ncorr(self.h) == c
            r = self.r = S.build_rows(n, dt, seed, nfree=nfree, free_all=free_all, finite_only=finite_only)
            for which, v in ((L.VEC_X, r["x0"]), (L.VEC_G, r["g"]), (L.VEC_LB, r["lb"]), (L.VEC_UB, r["ub"])):
                L.check(core.lbfgsx_upload(self.h, which, _p(np.ascontiguousarray(v, self.dt))))
            nf, no, dd = i64(), i64(), f64()
            wtd = np.full(80, np.nan)
            L.check(core.lbfgsx_b_cauchy_build(self.h, C.byref(nf), C.byref(no), C.byref(dd), _p(wtd)))
            na, nfr = i64(), i64()
            L.check(core.lbfgsx_b_cauchy_finish(self.h, 1.0, 1.0, 0, C.byref(na), C.byref(nfr)))
            assert (na.value, nfr.value) == (int(r["newact"].sum()), int(r["free"].sum()))
            L.check(core.lbfgsx_b_sub_begin(self.h))
            # the rows that are to have l == u: x0 moved away after the search (subspace_ref.build_rows, K_EQ)
            L.check(core.lbfgsx_upload(self.h, L.VEC_X, _p(np.ascontiguousarray(r["x0_sweep"], self.dt))))
            st = self.state()
            want = np.where(r["free"], S.ST_FREE, np.where(r["newact"], S.ST_NEWACT, 0)).astype(np.uint8)
            assert np.array_equal(st, want), "state bytes differ from the intended sets in %d rows" % int((st != want).sum())
            x0, g, lb, ub, drt = (self.vec(w) for w in (L.VEC_X, L.VEC_G, L.VEC_LB, L.VEC_UB, L.VEC_D))
            assert S.same_bits(x0, r["x0_sweep"]) and S.same_bits(lb, r["lb"]) and S.same_bits(ub, r["ub"]) and S.same_bits(g, r["g"])
            sub = {k: self.sub_down(i) for i, k in enumerate(S.SV_NAMES)}
            self.V = S.Vecs(dt, x0=x0, g=g, lb=lb, ub=ub, drt=drt, st=st, **sub)
            self.free = r["free"]
            self.gen = 0
            # what the host keeps about the list (csrc/lbfgsb_subspace.hip): a pass lists only when the partition before it
            # found at most kLuMax rows, and the list is valid when it fits lu_cap = min(n, 2^20)
            self.lu_pred, self.lu_cap, self.has_list = 1 << 40, min(n, 1 << 20), False
        except BaseException:
            self.close()
            raise

    def close(self):
        if self.h:
            self.core.lbfgsx_destroy(self.h)
            self.h = None

    # ---- copies
    def vec(self, which):
        a = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, _p(a)))
        return a

    def state(self):
        st = np.empty(self.n, np.uint8)
        self.L.check(self.core.lbfgsx_b_download_state(self.h, _p(st)))
        return st

    def sub_down(self, which):
        a = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_b_sub_download(self.h, which, _p(a)))
        return a

    def sub_up(self, which, a):
        a = np.ascontiguousarray(a, self.dt)
        assert np.isfinite(a).all()
        self.L.check(self.core.lbfgsx_b_sub_upload(self.h, which, _p(a)))
        setattr(self.V, S.SV_NAMES[which], a.copy())

    def fill(self, **given):
        """every sub-vector gets fresh sentinels (another generation each time: a stale value of an earlier call cannot pass for
        this call's), then the given arrays on the free rows"""
        self.gen += 1
        for which, name in enumerate(S.SV_NAMES):
            a = S.sentinel(which, self.n, self.dt, self.gen)
            if name in given:
                a[self.free] = np.asarray(given[name], self.dt)[self.free]
            self.sub_up(which, a)

    def edge(self, shift, **more):
        y, lam, mu = S.edge_values(self.V.li, self.V.ui, self.free, self.dt, shift, self.n + shift)
        rng = np.random.default_rng([self.n, shift, 17])
        self.fill(y=y, lam=lam, mu=mu, cF=more.pop("cF", rng.standard_normal(self.n)), **more)

    def list_rows(self):
        """the index list of L u U, or None when the context holds none"""
        rows = np.full(self.n + 1, -7, np.int32)
        cnt = i64(-5)
        self.L.check(self.core.lbfgsx_b_lu_list_download(self.h, _p(rows), self.n + 1, C.byref(cnt)))
        if cnt.value < 0:
            assert cnt.value == -1 and (rows == -7).all()
            return None
        assert (rows[cnt.value:] == -7).all()
        return rows[:cnt.value].copy()

    def verify(self, what):
        """all six vectors, drt and the state bytes against the mirror, over all rows"""
        V = self.V
        got = {k: self.sub_down(i) for i, k in enumerate(S.SV_NAMES)}
        got["drt"] = self.vec(self.L.VEC_D)
        for k, a in got.items():
            ref = getattr(V, k)
            if not S.same_bits(a, ref):
                bad = S.diff_rows(a, ref)
                i = int(bad[0])
                raise AssertionError("%s: %s differs in %d rows, first row %d (state %d, free %s): got %r, reference %r" % (
                    what, k, bad.size, i, V.st[i], bool(self.free[i]), a[i], ref[i]))
        st = self.state()
        if not np.array_equal(st, V.st):
            bad = np.nonzero(st != V.st)[0]
            raise AssertionError("%s: state byte differs in %d rows, first row %d: got %d, reference %d" % (
                what, bad.size, int(bad[0]), st[bad[0]], V.st[bad[0]]))

    def verify_drt(self, what):
        got = self.vec(self.L.VEC_D)
        assert S.same_bits(got, self.V.drt), "%s: drt differs in rows %s" % (what, S.diff_rows(got, self.V.drt)[:8])

    def _listed(self, nlu):
        """the bookkeeping of a pass that lists the new L u U"""
        cap = self.lu_cap if self.lu_pred <= 262144 else 0
        self.has_list = cap > 0 and nlu <= cap
        self.lu_pred = nlu

    def verify_list(self, what, present=None):
        lst = self.list_rows()
        if present is None:
            present = self.has_list
        else:
            assert present == self.has_list, "%s: the test expects %s list, the dispatch rules %s" % (
                what, "a" if present else "no", "one" if self.has_list else "none")
        if not present:
            assert lst is None, what + ": a list where none can be valid"
            return None
        assert lst is not None, what + ": no index list"
        want = np.nonzero(self.V.rows(S.ST_L | S.ST_U))[0]
        assert lst.size == want.size, "%s: the list holds %d rows, L u U has %d" % (what, lst.size, want.size)
        srt = np.sort(lst)
        assert (np.diff(srt) > 0).all(), what + ": a row is listed twice"
        assert np.array_equal(srt, want), what + ": the list is not the set of rows with ST_L | ST_U"
        return lst

    # ---- entries, each followed by the same statement on the mirror
    def partition(self):
        a, b, c_ = i64(), i64(), i64()
        self.L.check(self.core.lbfgsx_b_sub_partition(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        assert (a.value, b.value, c_.value) == S.partition(self.V), "sub_partition counts"
        self.has_list = False

    def check(self):
        cnt = (i64 * 4)()
        self.L.check(self.core.lbfgsx_b_sub_check(self.h, C.cast(cnt, vp)))
        assert list(cnt) == S.check(self.V), "sub_check counts"

    def sweep_begin(self, first):
        a, b, c_ = i64(), i64(), i64()
        cnt = (i64 * 4)()
        self.L.check(self.core.lbfgsx_b_sub_sweep_begin(self.h, first, C.byref(a), C.byref(b), C.byref(c_), C.cast(cnt, vp)))
        z = np.zeros(self.n, self.dt)
        ref = S.sweep(self.V, bool(first), None, z if first else None, z if first else None)
        got = [a.value, b.value, c_.value] + list(cnt)
        assert got == ref, "sub_sweep_begin(first = %d) counts %r, reference %r" % (first, got, ref)
        self._listed(ref[0] + ref[1])
        return ref

    def sub_op(self, op):
        self.L.check(self.core.lbfgsx_b_sub_op(self.h, op))
        S.sub_op(self.V, op)

    def wcombine(self, mode, mask, sel, coef, theta):
        self.L.check(self.core.lbfgsx_b_wcombine(self.h, mode, mask, sel, _p(coef), theta))
        S.wcombine(self.V, self.cols, mode, mask, sel, coef, theta)

    def judge(self, got, v, rows, what):
        ws = B.wtv_sums(self.cols, v, rows)
        B.judge(got, ws.exact, ws.bound, self.dt, 0, what)

    def solve_wty(self, pmask, sel, coef, theta, fmask):
        wty = np.full(self.t, np.nan)
        rc = self.core.lbfgsx_b_solve_wty(self.h, pmask, sel, _p(coef), theta, fmask, _p(wty))
        if rc:
            return rc
        S.solve(self.V, self.cols, self.V.rows(pmask), sel, coef, theta)
        self.judge(wty, self.V.y, self.V.rows(fmask), "solve_wty(pmask %d)" % pmask)
        return 0

    def solve_sweep(self, first, sel, coef, theta, c1=None, c2=None, rhs_entry=False):
        wty = np.full(self.t, np.nan)
        sums = (i64 * 7)()
        if rhs_entry:
            rc = self.core.lbfgsx_b_solve_sweep_rhs(self.h, first, sel, _pd(coef), theta, _pd(c1), _pd(c2), _pd(wty), C.byref(sums))
        else:
            rc = self.core.lbfgsx_b_solve_sweep(self.h, first, sel, _p(coef), theta, _p(wty), C.cast(sums, vp))
        if rc:
            return rc, None
        self.listed = self.V.rows(S.ST_L | S.ST_U)     # the rows lbfgsx_b_lu_sweep will walk
        ref, yd = S.solve_sweep(self.V, self.cols, first, sel, coef, theta, c1, c2)
        assert list(sums) == ref, "solve_sweep(first = %d) sums %r, reference %r" % (first, list(sums), ref)
        if not first:
            self.judge(wty, yd, self.free, "solve_sweep wty")
            self.pending = ref[0] + ref[1]
        else:
            assert np.isnan(wty).all(), "wty written by a first solve"
            self._listed(ref[0] + ref[1])
        return 0, ref

    def lu_sweep(self, coef, theta):
        sums = (i64 * 7)()
        rc = self.core.lbfgsx_b_lu_sweep(self.h, _p(coef), theta, C.cast(sums, vp))
        if rc:
            return rc, None
        ref = S.lu_sweep(self.V, self.cols, coef, theta, self.listed)
        assert list(sums) == ref, "lu_sweep sums %r, reference %r" % (list(sums), ref)
        self.lu_pred = self.pending + ref[0] + ref[1]
        self.has_list = self.lu_pred <= self.lu_cap
        return 0, ref

    def wtv_lu(self, with_c):
        t = self.t
        ol, ou, dd = np.full(t, np.nan), np.full(t, np.nan), np.full(2 * t, np.nan)
        zl, zu = i64(-1), i64(-1)
        if with_c:
            rc = self.core.lbfgsx_b_wtv_lu_c(self.h, _pd(ol), C.byref(zl), _pd(ou), C.byref(zu), _pd(dd))
        else:
            rc = self.core.lbfgsx_b_wtv_lu(self.h, _p(ol), C.byref(zl), _p(ou), C.byref(zu))
        if rc:
            return rc
        V = self.V
        for got, nnz, rows, v, nm in ((ol, zl, V.rows(S.ST_L), V.li, "out_l"), (ou, zu, V.rows(S.ST_U), V.ui, "out_u")):
            vv = np.where(rows, v, self.dt(0))            # an infinite bound never sits on a row of its own set
            self.judge(got, vv, rows, "wtv_lu " + nm)
            assert nnz.value == int(np.count_nonzero(vv[rows])), "wtv_lu nnz of " + nm
        if with_c:
            deliver = self.split and self.rhs_identity
            if not deliver:
                assert np.isnan(dd[0]), "negc_dd must be marked undeliverable here"
            else:
                rows = V.rows(S.ST_L | S.ST_U)
                ws = B.wtv_sums(self.cols, -V.cF, rows)
                for k in range(t):
                    B.check_pair(dd[2 * k], dd[2 * k + 1], ws.exact[k], B.dd_bound(ws.nrows, B.abs_wtv([self.cols[k]], V.cF, rows)[0]),
                                 "negc_dd[%d]" % k)
        return 0

    split, rhs_identity = True, True


def _ctx(lib, *a, **k):
    return Sub(lib, *a, **k)


def _coef(t, seed, scale=0.3):
    return scale * np.random.default_rng([seed, t]).standard_normal(max(t, 1))[:t] if t else None


# ---------------------------------------------------------------- partition, check, sweep_begin, sub_op
def _w(dt):
    return 2 if dt == F64 else 4


def _row_counts(dt):
    w = _w(dt)
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, 256 * w - 1, 256 * w + 1, 1024 * 256 * w + 256 * w + 1]


@pytest.mark.parametrize("dt,n", [(dt, n) for dt in (F64, F32) for n in _row_counts(dt)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_partition_rows(lib, dt, n):
    cx = _ctx(lib, n, 1, dt, 21)
    try:
        big = n >= 255
        cx.edge(0)
        if big:
            assert not set(S.EDGE_LABELS) - S.edge_classes(cx.V.li, cx.V.ui, cx.free, cx.V.y, cx.V.lam, cx.V.mu)
        cx.partition()
        cx.verify("sub_partition")
        cx.verify_list("after sub_partition", present=False)
        cx.check()
        cx.verify("sub_check changes nothing")
        cx.edge(7)                      # the same state bytes, every row in another class
        cx.check()
        # the sweeps: a fresh context keeps no list in its first one (the size before is unknown), the next ones keep it
        cx.edge(0)
        cx.sweep_begin(1)
        cx.verify("sub_sweep_begin(1)")
        cx.verify_list("first sweep of a context", present=False)
        before = cx.V.st.copy()
        cx.edge(7)
        cx.sweep_begin(0)
        cx.verify("sub_sweep_begin(0)")
        cx.verify_list("sub_sweep_begin(0)", present=None if n > (1 << 19) else True)   # the large n: by the rule of the sizes
        if big:
            assert S.transitions(before, cx.V.st) >= {"L->P", "U->P", "P->L", "P->U", "L->U"}
        cx.edge(3)
        cx.sweep_begin(1)
        cx.verify("sub_sweep_begin(1) again")
        cx.verify_list("sub_sweep_begin(1) again", present=None if n > (1 << 19) else True)
        for op in range(6):
            cx.edge(op + 1, yfb=S.edge_values(cx.V.li, cx.V.ui, cx.free, dt, op + 11, 5)[0])
            cx.sub_op(op)
            cx.verify("sub_op(%d)" % op)
    finally:
        cx.close()


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["all_lu", "no_lu"])
def test_all_or_none(lib, dt, mode):
    """every free row in L u U (nP = 0) and no row in L u U, partition and both sweeps; n = 1501, every row free in one run"""
    for free_all in (False, True):
        cx = _ctx(lib, 1501, 1, dt, 22, free_all=free_all)
        try:
            li, ui = cx.V.li, cx.V.ui
            finl, finu = np.isfinite(li), np.isfinite(ui)
            with np.errstate(invalid="ignore"):
                inside = np.where(finl & finu, li + (ui - li) * dt(0.5), np.where(finl, li + dt(1), np.where(finu, ui - dt(1), dt(0))))
                eqrow = li == ui
                # all_lu: below l where l is finite, above u else; rows without a finite bound cannot leave P: keep them out
                outside = np.where(finl, li - dt(1), np.where(finu, ui + dt(1), dt(0)))
            y = inside if mode == "no_lu" else outside
            one = np.ones(cx.n, dt)
            lam = -one if mode == "no_lu" else one       # no_lu: a row with l == u == y goes to P only with both multipliers < 0
            mu = lam
            for step in range(3):
                cx.fill(y=y, lam=lam, mu=mu, cF=np.random.default_rng(step).standard_normal(cx.n))
                if step == 0:
                    cx.partition()
                    cnt = [int(cx.V.rows(b).sum()) for b in (S.ST_L, S.ST_U, S.ST_P)]
                else:
                    cnt = cx.sweep_begin(1 if step == 1 else 0)
                cx.verify("%s step %d" % (mode, step))
                nofin = int((cx.free & ~finl & ~finu).sum())
                if mode == "no_lu":
                    # the first sweep takes zero multipliers: its l == u rows go to L
                    lu = int((cx.free & eqrow).sum()) if step == 1 else 0
                    assert cnt[0] + cnt[1] == lu and cnt[2] == int(cx.free.sum()) - lu
                else:
                    assert cnt[2] == nofin and cnt[0] + cnt[1] == int(cx.free.sum()) - nofin
                if step == 2:
                    cx.verify_list("%s sweep" % mode)
        finally:
            cx.close()


# ---------------------------------------------------------------- wcombine
HIST = [0, 1, 4, 5, 8, 10, 13, 20, 40]
N_HIST = 1501


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", HIST)
def test_wcombine(lib, dt, c):
    cx = _ctx(lib, N_HIST, c, dt, 23)
    try:
        coef = _coef(cx.t, 1)
        for with_list in (False, True):
            cx.edge(0)
            if with_list:
                cx.sweep_begin(1)
                cx.edge(7)
                cx.sweep_begin(0)
                cx.verify_list("wcombine set-up")
            else:
                cx.partition()
                cx.verify_list("wcombine set-up", present=False)
            assert cx.V.rows(S.ST_L).any() and cx.V.rows(S.ST_U).any() and cx.V.rows(S.ST_P).any()
            for mode in range(5):
                # the bound selectors on the rows of their own set, where the bound is finite (finite inputs only)
                masks = {S.CB_LINEAR: {S.ST_FREE: [S.VS_DRT]},
                         S.CB_SOLVE: {S.ST_FREE: [S.VS_NEG_CF], S.ST_P: [S.VS_DRT, S.VS_NEG_CF, S.VS_NEG_RHS, S.VS_Y],
                                      S.ST_L: [S.VS_NEG_RHS, S.VS_LBOUND], S.ST_U: [S.VS_UBOUND]},
                         S.CB_RHS_ADD: {S.ST_P: [S.VS_DRT]}, S.CB_LAMBDA: {S.ST_L: [S.VS_DRT], S.ST_L | S.ST_U: [S.VS_DRT]},
                         S.CB_MU: {S.ST_U: [S.VS_DRT]}}[mode]
                for mask, sels in masks.items():
                    for cf in ((None, coef) if c else (None,)):
                        for sel in sels:
                            # keep the state bytes, refresh the vectors (sentinels of a new generation outside the free rows)
                            rng = np.random.default_rng([mode, mask, sel])
                            cx.fill(**{k: rng.standard_normal(cx.n) for k in S.SV_NAMES})
                            cx.wcombine(mode, mask, sel, cf, THETA)
                            cx.verify("wcombine(mode %d, mask %d, sel %d, coef %s, list %s)" % (mode, mask, sel, cf is not None, with_list))
        assert cx.core.lbfgsx_b_wcombine(cx.h, 5, S.ST_FREE, 0, None, 1.0) == E_INVALID
        assert cx.core.lbfgsx_b_wcombine(cx.h, -1, S.ST_FREE, 0, None, 1.0) == E_INVALID
        cx.verify("refused wcombine")
    finally:
        cx.close()


# ---------------------------------------------------------------- solve_wty
@pytest.mark.parametrize("dt,n,c", [(dt, N_HIST, c) for dt in (F64, F32) for c in (1, 4, 5, 8, 10, 13, 16)] +
                         [(F64, 512 * 256 * 2 + 513, 2), (F32, 512 * 256 * 4 + 1025, 1)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_solve_wty(lib, dt, n, c):
    cx = _ctx(lib, n, c, dt, 24)
    try:
        coef = _coef(cx.t, 2)
        cx.edge(0)
        cx.partition()
        rng = np.random.default_rng(4)
        for pmask, fmask in ((S.ST_FREE, S.ST_FREE), (S.ST_P, S.ST_FREE)):
            for cf, sel in ((coef, S.VS_NEG_CF), (None, S.VS_NEG_RHS), (coef, S.VS_DRT)):
                cx.fill(**{k: rng.standard_normal(cx.n) for k in S.SV_NAMES})
                assert cx.solve_wty(pmask, sel, cf, THETA, fmask) == 0
                cx.verify("solve_wty(pmask %d, sel %d)" % (pmask, sel))
    finally:
        cx.close()


def test_solve_wty_refuses_more_than_32_columns(lib):
    cx = _ctx(lib, 300, 20, F64, 25)
    try:
        cx.edge(0)
        cx.partition()
        assert cx.solve_wty(S.ST_FREE, S.VS_NEG_CF, _coef(40, 1), THETA, S.ST_FREE) == E_INVALID
        cx.verify("refused solve_wty")
    finally:
        cx.close()


# ---------------------------------------------------------------- the fused sweeps
def _prepare_list(cx):
    """a fresh context keeps no list (the size of L u U before is unknown): two plain sweeps with a small L u U make one"""
    cx.edge(0)
    cx.sweep_begin(1)
    cx.verify_list("first sweep of a context", present=False)
    cx.edge(7)
    cx.sweep_begin(0)
    cx.verify_list("second sweep")


def _fused_sequence(cx, tie, inspect, end="verify"):
    """solve_sweep(first = 1) -> wtv_lu[_c] -> three times (solve_sweep[_rhs](first = 0) -> lu_sweep) -> ASSIGN_Y.
    tie: no coefficients and theta = 1; cF = -(an edge input) before the first solve, rhs = -(another edge input) before each
         later one, so y lands on the bounds exactly and sweep_row_v decides every tie with zero multipliers; cF = -y + d,
         d = 0, > 0, < 0 by row, before each lu_sweep, so the multipliers there come out +0, > 0 and < 0 (rows leave L and U,
         rows with l == u go L -> U).  Needs inspect (the uploads).
    inspect: the vectors are downloaded after every step; else only the list, the sums and the counts are looked at on the
         way and the vectors at the end -- end = "verify": all of them, then ASSIGN_Y; end = "assign": ASSIGN_Y first (on live
         compact vectors it assigns from them and writes nothing else back), then drt alone."""
    n, t, dt = cx.n, cx.t, cx.dt
    assert inspect or not tie
    theta = 1.0 if tie else THETA
    rng = np.random.default_rng([n, t, 5])
    li, ui = cx.V.li, cx.V.ui
    y0 = S.edge_values(li, ui, cx.free, dt, 4, 9)[0]
    cF = -y0 if tie else (-THETA * y0 + 0.05 * rng.standard_normal(n))
    cx.fill(cF=cF, y=rng.standard_normal(n), lam=rng.standard_normal(n), mu=rng.standard_normal(n))
    rc, s0 = cx.solve_sweep(1, S.VS_NEG_CF, None if tie else _coef(t, 3, 0.02), theta)
    assert rc == 0
    if inspect:
        cx.verify("solve_sweep(first = 1)")
    cx.verify_list("solve_sweep(first = 1)")
    assert s0[0] > 0 and s0[1] > 0 and s0[2] > 0 and s0[3] > 0
    lu_ok = 0 if (cx.split or t <= 24) else E_INVALID      # k_multidot_list2 exists up to 24 columns
    assert cx.wtv_lu(False) == lu_ok
    assert cx.wtv_lu(True) == lu_ok
    ready = cx.core.lbfgsx_b_solve_sweep_rhs_ready(cx.h)
    assert ready == (1 if (cx.split and cx.rhs_identity) else 0)
    seen = set()
    for it, (a1, a2) in enumerate(((3, None), (None, 4), (5, 6))):
        c1 = None if a1 is None or tie else _coef(t, a1, 0.05)
        c2 = None if a2 is None or tie else _coef(t, a2, 0.05)
        use_rhs = bool(ready) and not tie
        assert inspect or use_rhs
        if tie:
            cx.sub_up(S.SV_RHS, np.where(cx.free, -S.edge_values(li, ui, cx.free, dt, 9 + 5 * it, 3)[0], cx.V.rhs))
        elif not use_rhs:
            # the pass of its own a caller without the fused rhs updates makes (test_gp_rhs): here through the upload
            W = cx.V.copy()
            S.gp_rhs(W, cx.cols, W.rows(S.ST_P), c1, c2)
            cx.sub_up(S.SV_RHS, W.rhs)
            c1 = c2 = None
        old = cx.verify_list("before sweep %d" % it)
        before = cx.V.st.copy()
        rc, s1 = cx.solve_sweep(0, S.VS_NEG_RHS, None if tie else _coef(t, 7 + it, 0.02), theta, c1, c2, rhs_entry=use_rhs)
        assert rc == 0
        now = cx.list_rows()
        assert now is not None and np.array_equal(now, old), "the list changed before lbfgsx_b_lu_sweep"
        if inspect:
            cx.verify("solve_sweep(first = 0), sweep %d" % it)
        if tie:
            d = np.array([0.0, 0.5, -0.5])[(np.arange(n) + it) % 3]
            cx.sub_up(S.SV_CF, np.where(cx.listed, -cx.V.y + d, cx.V.cF))
        rc, s2 = cx.lu_sweep(None if tie else _coef(t, 11 + it, 0.05), theta)
        assert rc == 0
        if inspect:
            cx.verify("lu_sweep, sweep %d" % it)
        cx.verify_list("lu_sweep, sweep %d" % it)
        tot = [a + b for a, b in zip(s1, s2)]
        assert tot[:3] == [int(cx.V.rows(b).sum()) for b in (S.ST_L, S.ST_U, S.ST_P)]
        seen |= S.transitions(before, cx.V.st)
    if n >= 255:
        want = {"P->L", "P->U", "L->P", "U->P"} | ({"L->U"} if tie else set())
        assert seen >= want, "the sweeps made only the set changes %s" % sorted(seen)
    if end == "verify":
        cx.verify("the end of the sweeps")
        cx.sub_op(S.SO_ASSIGN_Y)
        cx.verify("ASSIGN_Y")
    else:
        cx.sub_op(S.SO_ASSIGN_Y)
        cx.verify_drt("ASSIGN_Y from the compact vectors")


SWEEP_CS = [1, 4, 5, 8, 10, 12, 13, 20, 24, 30, 40]


@pytest.mark.parametrize("tie", [0, 1], ids=["coef", "tie"])
@pytest.mark.parametrize("dt,n,c", [(dt, N_HIST, c) for dt in (F64, F32) for c in SWEEP_CS] +
                         [(F64, n, 1) for n in (1, 2, 3, 63, 64, 65, 127, 129, 255, 257)] +
                         [(F64, 70001, 2), (F32, 70001, 2), (F64, 512 * 256 * 2 + 513, 1)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_fused_sweeps(lib, dt, n, c, tie):
    if tie and (n != N_HIST or c not in (1, 10, 40)):
        return   # the ties are decided by sweep_row_v whatever the class: three classes, both types
    cx = _ctx(lib, n, c, dt, 26)
    try:
        _prepare_list(cx)
        if n < 255:
            _small_fused(cx)
        else:
            _fused_sequence(cx, bool(tie), inspect=True)
    finally:
        cx.close()


def _small_fused(cx):
    """a handful of rows: the sets may be empty, a sweep may find no list to walk; whatever the entries answer must match"""
    rng = np.random.default_rng(cx.n)
    y0 = S.edge_values(cx.V.li, cx.V.ui, cx.free, cx.dt, 12, 9)[0]
    cx.fill(cF=-THETA * y0, y=rng.standard_normal(cx.n), lam=rng.standard_normal(cx.n), mu=rng.standard_normal(cx.n))
    rc, s0 = cx.solve_sweep(1, S.VS_NEG_CF, _coef(cx.t, 3, 0.02), THETA)
    assert rc == 0
    cx.verify("solve_sweep(first = 1)")
    lst = cx.verify_list("solve_sweep(first = 1)")
    rc, s1 = cx.solve_sweep(0, S.VS_NEG_RHS, _coef(cx.t, 4, 0.02), THETA)
    if lst.size == 0:
        assert rc == E_INVALID          # no row to walk: the caller runs the separate passes
        cx.verify("refused solve_sweep")
        return
    assert rc == 0
    cx.verify("solve_sweep(first = 0)")
    rc, s2 = cx.lu_sweep(_coef(cx.t, 5, 0.05), THETA)
    assert rc == 0
    cx.verify("lu_sweep")
    cx.verify_list("lu_sweep")


@pytest.mark.parametrize("dt,c", [(F64, 4), (F64, 8), (F64, 10), (F64, 12), (F64, 16), (F32, 10)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_fused_sweeps_one_lane(lib, monkeypatch, dt, c):
    """LBFGSX_SPLIT=0: k_solve_sweep<NC = 8, 16, 20, 24, 32>, k_multidot_list2; no fused rhs updates, negc_dd undeliverable"""
    monkeypatch.setenv("LBFGSX_SPLIT", "0")
    cx = _ctx(lib, N_HIST, c, dt, 27)
    cx.split = False
    try:
        _prepare_list(cx)
        _fused_sequence(cx, False, inspect=True)
    finally:
        cx.close()


def test_one_lane_refuses_more_than_32_columns(lib, monkeypatch):
    monkeypatch.setenv("LBFGSX_SPLIT", "0")
    cx = _ctx(lib, 600, 20, F64, 28)
    try:
        _prepare_list(cx)
        cx.edge(2)
        lst = cx.list_rows()
        rc, _ = cx.solve_sweep(1, S.VS_NEG_CF, _coef(40, 1), THETA)
        assert rc == E_INVALID
        assert cx.wtv_lu(False) == E_INVALID       # 2c > 24 without the split-row kernels
        cx.verify("refused entries")
        assert np.array_equal(cx.list_rows(), lst)
    finally:
        cx.close()


def test_rhs_identity_off_marks_negc_dd(lib, monkeypatch):
    monkeypatch.setenv("LBFGSX_RHS_IDENTITY", "0")
    cx = _ctx(lib, N_HIST, 4, F64, 29)
    cx.rhs_identity = False
    try:
        _prepare_list(cx)
        assert cx.core.lbfgsx_b_solve_sweep_rhs_ready(cx.h) == 0
        assert cx.wtv_lu(True) == 0
    finally:
        cx.close()


# ---------------------------------------------------------------- LBFGSX_GP_RHS
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("dt,c", [(F64, 1), (F64, 4), (F64, 10), (F64, 13), (F32, 5), (F64, 40)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_gp_rhs(lib, monkeypatch, split, dt, c):
    if not split and 2 * c + 1 > 31:
        return   # the one-lane v row exists up to 30 columns
    monkeypatch.setenv("LBFGSX_SPLIT", str(split))
    cx = _ctx(lib, N_HIST, c, dt, 30)
    try:
        t = cx.t
        cx.edge(0)
        cx.partition()
        rng = np.random.default_rng(6)
        for mask in (S.ST_P, S.ST_FREE):
            for c1, c2 in ((_coef(t, 1), None), (None, _coef(t, 2)), (_coef(t, 1), _coef(t, 2))):
                for entry in ("wtv_prologue", "gram_fused_ex"):
                    cx.fill(**{k: rng.standard_normal(cx.n) for k in S.SV_NAMES})
                    w = np.full(t, np.nan)
                    if entry == "wtv_prologue":
                        rc = cx.core.lbfgsx_b_wtv_prologue(cx.h, mask, S.VS_NEG_RHS, S.GP_RHS, _p(c1), _p(c2), _p(w))
                    else:
                        G = np.full((t, t), np.nan)
                        rc = cx.core.lbfgsx_b_gram_fused_ex(cx.h, mask, S.VS_NEG_RHS, S.GP_RHS, _p(c1), _p(c2), _p(G), _p(w))
                    cx.L.check(rc)
                    rows = cx.V.rows(mask)
                    S.gp_rhs(cx.V, cx.cols, rows, c1, c2)
                    what = "%s GP_RHS(mask %d, c1 %s, c2 %s)" % (entry, mask, c1 is not None, c2 is not None)
                    cx.verify(what)
                    ws = B.wtv_sums(cx.cols, -cx.V.rhs, rows)
                    B.judge(w, ws.exact, ws.bound, F64, 0, what)        # the one-pass Gram family stores doubles
    finally:
        cx.close()


# ---------------------------------------------------------------- refusals
def test_refusals(lib):
    cx = _ctx(lib, 700, 3, F64, 31)
    core = cx.core
    try:
        cx.edge(0)
        cx.partition()                                   # a partition that keeps no list
        cx.verify_list("after sub_partition", present=False)
        rc, _ = cx.solve_sweep(0, S.VS_NEG_RHS, _coef(6, 1), THETA)
        assert rc == E_INVALID
        assert cx.wtv_lu(False) == E_INVALID and cx.wtv_lu(True) == E_INVALID
        rc, _ = cx.lu_sweep(_coef(6, 1), THETA)
        assert rc == E_INVALID
        cx.verify("refusals without a list")
        cx.verify_list("still none", present=False)
        _prepare_list(cx)
        lst = cx.list_rows()
        rc, _ = cx.lu_sweep(_coef(6, 1), THETA)          # nothing pending
        assert rc == E_INVALID
        for first in (1, 0):
            for sel in (S.VS_LBOUND, S.VS_UBOUND):
                rc, _ = cx.solve_sweep(first, sel, _coef(6, 1), THETA)
                assert rc == E_INVALID
        rc, _ = cx.solve_sweep(1, S.VS_NEG_RHS, _coef(6, 1), THETA, _coef(6, 2), None, rhs_entry=True)   # rhs updates ride on first = 0 only
        assert rc == E_INVALID
        rc, _ = cx.solve_sweep(0, S.VS_NEG_CF, _coef(6, 1), THETA, _coef(6, 2), None, rhs_entry=True)    # ... and on v = -rhs only
        assert rc == E_INVALID
        cx.verify("refusals with a list")
        assert np.array_equal(cx.list_rows(), lst)
        # the inspection entries themselves
        a = np.zeros(cx.n)
        assert core.lbfgsx_b_sub_download(cx.h, 6, _p(a)) == E_INVALID and core.lbfgsx_b_sub_download(cx.h, -1, _p(a)) == E_INVALID
        assert core.lbfgsx_b_sub_upload(cx.h, 6, _p(a)) == E_INVALID and core.lbfgsx_b_sub_upload(cx.h, S.SV_Y, None) == E_INVALID
        assert core.lbfgsx_b_sub_download(cx.h, S.SV_Y, None) == E_INVALID
        cnt = i64(0)
        small = np.zeros(max(lst.size - 1, 1), np.int32)
        assert lst.size >= 2 and core.lbfgsx_b_lu_list_download(cx.h, _p(small), lst.size - 1, C.byref(cnt)) == E_INVALID
        cx.verify("refused inspection entries")
        assert np.array_equal(cx.list_rows(), lst)
    finally:
        cx.close()
    # no history: every entry over the 2c columns refuses
    cx = _ctx(lib, 300, 0, F64, 32)
    try:
        _prepare_list(cx)
        rc, _ = cx.solve_sweep(1, S.VS_NEG_CF, None, THETA)
        assert rc == E_INVALID
        assert cx.wtv_lu(False) == E_INVALID and cx.solve_wty(S.ST_FREE, S.VS_NEG_CF, None, THETA, S.ST_FREE) == E_INVALID
        cx.verify("refusals without history")
    finally:
        cx.close()
    # a context that is not bounded
    h = vp()
    L = cx.L
    L.check(core.lbfgsx_create(C.byref(h), L.F64, 100, 3, 0, 0))
    try:
        a = np.zeros(100)
        cnt = i64(0)
        assert core.lbfgsx_b_sub_download(h, S.SV_Y, _p(a)) == E_INVALID and core.lbfgsx_b_sub_upload(h, S.SV_Y, _p(a)) == E_INVALID
        assert core.lbfgsx_b_lu_list_download(h, _p(a), 100, C.byref(cnt)) == E_INVALID
    finally:
        core.lbfgsx_destroy(h)


# ---------------------------------------------------------------- the index list: buffer and thresholds
def _sweep_with(cx, out_rows, first):
    """a plain sweep with y one unit outside a finite bound on the rows `out_rows` (indices) and inside on every other row;
    multipliers < 0, so that a row with l == u == y stays out of L and U in a later sweep (a first sweep takes zero
    multipliers and puts it into L).  Every free row of these contexts has a finite bound."""
    li, ui = cx.V.li, cx.V.ui
    finl = np.isfinite(li)
    assert (np.isfinite(li) | np.isfinite(ui))[cx.free].all() and cx.free[out_rows].all()
    with np.errstate(invalid="ignore"):
        y = np.where(finl & np.isfinite(ui), li + (ui - li) * cx.dt(0.5), np.where(finl, li + cx.dt(1), ui - cx.dt(1)))
        y[out_rows] = np.where(finl[out_rows], li[out_rows] - cx.dt(1), ui[out_rows] + cx.dt(1))
    m1 = -np.ones(cx.n, cx.dt)
    cx.fill(y=y, lam=m1, mu=m1, cF=(np.arange(cx.n) % 7).astype(cx.dt))
    return cx.sweep_begin(first)


@pytest.mark.parametrize("n", [1024, 4096, 1024 * 1024 + 1280], ids=str)
def test_lds_buffer(lib, n):
    """f32: a block of k_sub_sweep_begin walks 1024 rows up to the grid cap.  Every row free and finitely bounded.
    n = 1024 B with every row outside: every block's 1024-entry buffer exactly full.  n = 2^20 + 1280: blocks 0..4 walk a second
    stride and overflow their buffer by four wavefronts -- lu_flush_lds and the direct append both contribute; 2000 rows in
    the middle stay inside so that |L u U| fits lu_cap = 2^20."""
    cx = _ctx(lib, n, 1, F32, 33, free_all=True, finite_only=True)
    try:
        assert cx.free.all()
        _sweep_with(cx, np.arange(min(100, n)), 1)
        cx.verify_list("first sweep of a context", present=False)
        rows = np.arange(n) if n <= 4096 else np.concatenate([np.arange(500000), np.arange(502000, n)])
        cnt = _sweep_with(cx, rows, 0)
        assert cnt[0] + cnt[1] == rows.size
        cx.verify("sweep with full buffers")
        cx.verify_list("sweep with full buffers")
    finally:
        cx.close()


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_list_thresholds(lib, dt):
    """kLuMax = 262144: the list is kept iff the partition BEFORE found at most that many rows; lu_cap = min(n, 2^20): a list
    that overflows it is not valid and its dependants refuse.  The counts are exact in every case (asserted by sweep_begin)."""
    n = (1 << 20) + 4096
    cx = _ctx(lib, n, 1, dt, 34, free_all=True, finite_only=True)
    try:
        assert cx.free.all()
        _sweep_with(cx, np.arange(10), 1)          # the first sweep of the minimisation; the later ones decide exactly
        for before, now, kept in ((262144, 300000, True), (262145, 5000, False), (5000, (1 << 20) + 1, False), (1000, 1 << 20, True)):
            cnt = _sweep_with(cx, np.arange(before), 0)
            assert cnt[0] + cnt[1] == before
            cnt = _sweep_with(cx, np.arange(n - now, n), 0)
            assert cnt[0] + cnt[1] == now
            cx.verify_list("|L u U| = %d after %d" % (now, before), present=kept)
            if not kept:
                rc, _ = cx.solve_sweep(0, S.VS_NEG_RHS, _coef(2, 1), THETA)
                assert rc == E_INVALID and cx.wtv_lu(False) == E_INVALID
        cx.verify("the last sweep")
    finally:
        cx.close()


# ---------------------------------------------------------------- compact copy, compact vectors
def _compact_counts(core):
    out = (i64 * 4)()
    assert core.lbfgsx_b_compact_vec_counts(C.byref(out), 0) == 0
    return list(out)


def _full_pass(cx):
    """the full Gram pass of a first solve over ST_FREE with the compaction hint; returns the walked-compact-copy counters' change
    of the prologue pass that follows (1, nfree) when the copy was taken"""
    core, L = cx.core, cx.L
    L.check(core.lbfgsx_b_set_compaction(cx.h, 1))
    t = cx.t
    G, w, gd = np.full((t, t), np.nan), np.full(t, np.nan), np.full(t * (t + 1), np.nan)
    L.check(core.lbfgsx_b_gram_fused_dd(cx.h, S.ST_FREE, S.VS_NEG_CF, S.GP_NONE, None, None, _p(G), _p(w), _p(gd)))
    ws = B.wtv_sums(cx.cols, -cx.V.cF, cx.free)
    B.judge(w, ws.exact, ws.bound, F64, 0, "full pass wtv")
    cnt = (i64 * 8)()
    L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
    b4 = (cnt[4], cnt[5])
    w2 = np.full(t, np.nan)
    L.check(core.lbfgsx_b_wtv_prologue(cx.h, S.ST_FREE, S.VS_NEG_CF, S.GP_NONE, None, None, _p(w2)))
    L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
    B.judge(w2, ws.exact, ws.bound, F64, 0, "prologue pass wtv")
    return (cnt[4] - b4[0], cnt[5] - b4[1])


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,nfree,taken", [(6000, 4096, True), (6000, 4095, False), (8192, 7168, True), (8192, 7169, False)])
def test_compact_full_pass(lib, dt, n, nfree, taken):
    cx = _ctx(lib, n, 3, dt, 35, nfree=nfree)
    try:
        cx.fill(cF=np.random.default_rng(1).standard_normal(n))
        walked = _full_pass(cx)
        assert walked == ((1, nfree) if taken else (0, 0)), "compact copy %s" % ("not taken" if taken else "taken")
        cx.verify("the full pass changes no vector")
    finally:
        cx.close()


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["live_assign", "live_verify", "off", "download_mid"])
def test_compact_sweeps(lib, monkeypatch, dt, mode):
    """solve_sweep(first = 1) -> wtv_lu_c -> solve_sweep_rhs(first = 0) -> lu_sweep (three sweeps) -> sub_op(ASSIGN_Y) over the
    compact copy.  live_*: on live compact vectors -- only the list, the sums and the counts are looked at on the way; at the
    end either ASSIGN_Y runs on them (k_cv_back<1>; drt compared) or everything is downloaded first (k_cv_back<0>).  off:
    LBFGSX_COMPACT_VEC=0.  download_mid: the vectors are downloaded after every step, which puts them back at their rows
    right after the first solve.  The same reference for all four."""
    if mode == "off":
        monkeypatch.setenv("LBFGSX_COMPACT_VEC", "0")
    n, nfree = 6000, 4500
    cx = _ctx(lib, n, 3, dt, 36, nfree=nfree)
    try:
        _prepare_list(cx)
        cx.fill(cF=np.random.default_rng(1).standard_normal(n))
        assert _full_pass(cx) == (1, nfree)
        c0 = _compact_counts(cx.core)
        _fused_sequence(cx, False, inspect=(mode == "download_mid"), end="assign" if mode == "live_assign" else "verify")
        c1 = _compact_counts(cx.core)
        got = (c1[0] - c0[0], c1[1] - c0[1])     # minimisations started on compact vectors, times they were put back early
        want = {"live_assign": (1, 0), "live_verify": (1, 1), "off": (0, 0), "download_mid": (1, 1)}[mode]
        assert got == want, "compact vectors: (starts, early put-backs) = %r, intended %r" % (got, want)
    finally:
        cx.close()
