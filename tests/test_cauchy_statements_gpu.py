"""-m gpu: the device side of the generalized-Cauchy-point search against tests/cauchy_ref.py, which
tests/test_cauchy_ref_cpu.py proves against a scalar transcription of the reference, against the oracle and against wrong
variants of itself.  tests/test_gcp_device_gpu.py and tests/test_lbfgsb_gpu.py reach this phase through whole searches at
1e-10, or compare one device form with another; all forms share k_cauchy_build's row statement, the list appends, the
(key, row) order of the sorts, the gathers and k_cauchy_finish's row statement, so a wrong branch at t == t_cross, a tie group
in another order, a dropped tail row or a row lost when a block's list buffer overflows looks the same on both sides.  Here
every vector, state byte and sorted list is compared bit for bit over ALL n rows, every count and index exactly, d.d and the
W' sums with bounded_sums_ref.check_rounded, the search without stored pairs bit for bit against cauchy_ref.scan_emulate, the
search with stored pairs against the exact search within cauchy_ref.scan_bound, the exit index exactly.  No other tolerance.

Set-up through the ABI only (lbfgsx_upload, lbfgsx_bfgs_add_correction_host, lbfgsx_ls_begin / _ls_end); x, g, lb, ub are
downloaded and the references are fed with the downloaded values.  brk, d and the sorted row numbers are read through the
inspection entry lbfgsx_b_cauchy_download.  Finite inputs apart from infinite bounds: NaN handling is out of scope (a NaN
threshold of lbfgsx_b_cauchy_build_partial is an argument, not data: it selects the full sort).

Where the library departs from the reference on purpose: an f32 problem's search is gathered into doubles and its per-crossing
terms are computed in double; only the f' / f'' chains and the exit test run in float (gcp_chain_host<float>).
cauchy_ref.scan_emulate states exactly that.  Inside a group of equal break points the device's order is by row; the
reference's sort leaves any order there (the CPU test compares the oracle's order group-wise).

Entry points, kernels and the shapes that reach them (csrc/lbfgsb_cauchy.hip, lbfgsb_linesearch.hip, lbfgsb_kernels.cuh,
gcp_scan.cuh), W = 2 (f64) or 4 (f32), grid_for(n) = min(1024, ceil(floor(n / W) / 256)) blocks of 256:
  lbfgsx_b_cauchy_build, plain and after lbfgsx_b_force_bounds_deferred                       test_build_rows
      k_cauchy_build<T>: one row per thread and stride, so a block walks W rows at least; rocprim radix_sort_pairs over all n
      when nord > 0.  n = 1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 256 W - 1, 256 W + 1 and 1024 * 256 * W + 256 * W + 1
      (every block walks a further stride).  edge_rows: every class needs n >= cauchy_ref.EDGE_NEED (asserted on the CPU).
  lbfgsx_b_cauchy_finish                                                                      test_finish_rows
      k_cauchy_finish<T>: W rows per lane, tail rows by thread 0 of block 0; drt and the newly active list with the default,
      neither with LBFGSX_FINISH_FUSE=0.  The same n.
  lbfgsx_b_cauchy_chunk, lbfgsx_b_cauchy_sort_full                                            test_full_order
      k_cauchy_gather<T>, min(2048, ceil(count / 256)) blocks; the chunk of the first 512 launched ahead by
      lbfgsx_b_cauchy_build_partial (wtd given, ncorr > 0) is taken when first == 0, count == min(512, nsorted), idx == NULL.
      c = 0, 1, 4, 5, 10, 20, 40 with m = c and c + 3 pairs added (the ring has wrapped).
  lbfgsx_b_cauchy_build_partial                                                               test_partial_routes, test_partial_ties
      tau <= 0, inf, NaN: full radix sort.  First call with a finite tau: rocprim::select riding behind the build (default) or
      after a wait (LBFGSX_SYNC_MERGE=0) + k_gather_keys + radix_sort_pairs.  Second call: k_cauchy_build lists the candidates
      (lu_append_lds / lu_flush_lds); 1..4096 of them: k_psel_sort_small<T> (one block, P = 128..4096); more, or
      LBFGSX_PSEL_SMALL=0: radix_sort_keys of the rows (a copy for one row) + k_gather_keys + radix_sort_pairs;
      LBFGSX_SELECT_CAP below the count: rocprim::select again; LBFGSX_SELECT_INLINE=0: never listed.
  the blocks' list buffers (kListBuf = 1024)                                  test_list_buffers, test_newact_cap, test_compact_list_cap
      f32, every row a candidate, n = 1024 * 3 (every block's buffer exactly full) and n = 1024 * 1024 + 4096 * 70 (above the
      grid cap: k_cauchy_build walks one row per thread and stride of 1024 * 256 rows, so blocks 0..95 meet 1536 rows and the
      others 1280: buffer and direct append both contribute); LBFGSX_NEWACT_CAP = count,
      count - 1, 1 observed through lbfgsx_b_wtv(LBFGSX_VS_DRT, LBFGSX_ST_NEWACT); LBFGSX_WTD_LIST_CAP = count, count - 1, 1:
      the rows outside the kept compact copy (olist of k_cauchy_build, read by kx_multidot2_wf) through wtd, the deferred
      lbfgsx_b_correction_dots and lbfgsx_b_compact_vec_counts.
  lbfgsx_b_post_linesearch_build + lbfgsx_b_cauchy_build_partial                              test_post_build
      k_b_post_build<T> (W rows per lane, tail by thread 0); keys not written when the pass lists the candidates, so the
      sort_full after it runs k_keys_from_brk<T>.  Refused hand-overs: another tau, x moved, a row the clamp would move.
  lbfgsx_b_cauchy_scan                                                                        test_scan_no_pairs, test_scan_pairs,
      k_gcp_gather<T>, k_gcp_a1<NC>, k_gcp_tiles, k_gcp_a3b1<NC>, k_gcp_b3c1<NC, CHAIN>,      test_scan_two_calls, test_scan_refusals
      k_gcp_extract<NC>, and gcp_chain_host<CT> (default) or k_gcp_c3 (LBFGSX_GCP_CHAIN=scan).  NC by 2c: 4 (c = 0, 1, 2),
      8 (4), 12 (5), 16 (7, 8), 20 (10), 24 (12), 32 (16), 40 (20), 48 (24), 64 (32), 80 (40: the parked form).  Tiles of 256
      crossings; k_gcp_tiles takes 64 tiles a round (a second round from 64 * 256 + 1); from 2^17 crossings the host chain
      reads the chunk in kChainPieces = 8 pieces.

Smallest exact margin / bound on -f'/f'' over the group ends up to the exit, per committed case, host chain (the scan chain's
ratio is larger in every f64 case but exit0, 4.42e15, and tieflip, 2.17e13, and about 1e13 in the f32 cases, whose scan chain
runs in double), from tests/test_cauchy_ref_cpu.py::test_designed_exit_and_margins; the required factor is cauchy_ref.FACTOR = 4.
The designed exits stand 1e3 clear of a -f'/f'' of order 1, so the condition holds by a wide margin by construction and the
exit index does not react to moderate errors in f' and f'': those are what the bound checks on p, c, f', f'' catch.
  f64  c1 2.62e12  c2 2.48e12  c4 2.17e12  c5 1.98e12  c7 2.08e12  c8 1.76e12  c10 1.52e12  c12 2.74e12  c16 1.91e12  c20 1.35e12
       c24 1.48e12  c32 8.86e11  c40 3.6e11  exit0 4.47e15  exit255 8.14e12  exit256 8.25e12  tie300 2.58e13  noexit 5.68e12
       listend 5.67e12  tieflip 2.25e13
  f32  c1 4.84e3  c2 4.76e3  c4 4.0e3  c5 3.9e3  c7 4.09e3  c8 3.98e3  c10 3.1e3  c12 7.93e3  c16 5.47e3  c20 4.86e3  c24 4.41e3
       c32 2.98e3  c40 2.6e3  exit0 8.33e6  exit255 1.54e4  exit256 1.56e4  tie300 4.81e4  noexit 1.1e4  listend 1.09e4
       tieflip 8.92e4

  lbfgsx_test_cauchy_subspace(subspace = 0), empty history                                    test_whole_search
      Cauchy<Scalar>::get_cauchy_point: build_partial (tau = 0: full sort), the host loop over lbfgsx_b_cauchy_chunk up to
      sorted position LBFGSX_GCP_DEVICE_MIN (-1: to the end), lbfgsx_b_cauchy_scan from there, lbfgsx_b_cauchy_finish.
      n = 1, 2, 3 (every row on its bound), 63, 64, 65, 257, with edge_rows(extreme=False): the three classes whose quotient
      leaves the normal range (subnormal, underflow to 0, overflow to inf) are ordinary rows here -- next to g = 1e65 a whole
      search ends at its first crossing, where f' = -d.d + g^2 cancels; those classes are held by test_build_rows,
      test_finish_rows and test_partial_ties.  Without pairs every step is a fixed sequence of IEEE operations
      (cauchy_ref.whole_search): the crossing count, the state bytes AND xcp are compared bit for bit, so no margin condition
      is needed.  With pairs M comes from the library's own factorisation, which no entry exposes: not covered here.

Found by this file (test_post_build, "x moved"): lbfgsx_b_cauchy_build_partial took the break points that
lbfgsx_b_post_linesearch_build had computed ahead although lbfgsx_upload had rewritten x in between -- the hand-over checked the
buffer index, the threshold and the clamp, but nothing an upload changes.  The context now counts lbfgsx_upload / _fill /
_gen_rosen_x0 (ctx::vec_writes) and the hand-over is refused when the count has moved.  No solver path uploads between the two
calls, so no trajectory changed.

Not covered here: whole searches with stored pairs (M comes from the library's own factorisation, which no entry exposes)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import bounded_sums_ref as B
import cauchy_ref as G
import statement_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]
vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double
pd, pi64 = C.POINTER(f64), C.POINTER(i64)
E_INVALID = -1
VS_DRT, ST_NEWACT = 0, 2


@pytest.fixture(scope="module")
def lib():
    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1
    for name, args in (("lbfgsx_b_cauchy_build", [vp, pi64, pi64, pd, vp]),
                       ("lbfgsx_b_cauchy_build_partial", [vp, f64, pi64, pi64, pi64, pd, vp]),
                       ("lbfgsx_b_cauchy_sort_full", [vp]),
                       ("lbfgsx_b_cauchy_chunk", [vp, i64, i64, vp, vp, vp, vp, vp]),
                       ("lbfgsx_b_cauchy_scan", [vp, i64, i64, i64, vp, f64, f64, vp, pi64, vp]),
                       ("lbfgsx_b_cauchy_finish", [vp, f64, f64, i32, pi64, pi64]),
                       ("lbfgsx_b_force_bounds_deferred", [vp]), ("lbfgsx_b_download_state", [vp, vp]),
                       ("lbfgsx_b_wtv", [vp, i32, i32, vp, pi64]), ("lbfgsx_b_sub_begin", [vp]),
                       ("lbfgsx_b_set_compaction", [vp, i32]),
                       ("lbfgsx_b_gram_fused_dd", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                       ("lbfgsx_b_correction_dots", [vp, vp, vp]), ("lbfgsx_b_correction_dots_defer", [vp])):
        f = getattr(core, name)
        f.restype, f.argtypes = i32, args
    return core, L


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _w(dt):
    return 2 if dt == F64 else 4


def _row_counts(dt):
    w = _w(dt)
    return [1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 256 * w - 1, 256 * w + 1, 1024 * 256 * w + 256 * w + 1]


def _ids(v):
    return getattr(v, "__name__", str(v))


class Ctx:
    """one bounded context with the given rows (and pairs); the references are fed with what the device holds"""

    def __init__(self, lib, dt, x, g, lb, ub, pairs=(), m=None):
        self.core, self.L = lib
        core, L = lib
        self.dt, self.n = np.dtype(dt).type, x.size
        self.h = vp()
        L.check(core.lbfgsx_create(C.byref(self.h), L.F64 if dt == F64 else L.F32, self.n, max(m or len(pairs), 1), 0, L.FLAG_BOUNDED))
        try:
            for s_, y_ in pairs:
                L.check(core.lbfgsx_bfgs_add_correction_host(self.h, _p(np.ascontiguousarray(s_, self.dt)), _p(np.ascontiguousarray(y_, self.dt))))
            self.c = core.lbfgsx_bfgs_ncorr(self.h)
            for which, v in ((L.VEC_X, x), (L.VEC_G, g), (L.VEC_LB, lb), (L.VEC_UB, ub)):
                self.up(which, v)
            self.x, self.g, self.lb, self.ub = (self.vec(w) for w in (L.VEC_X, L.VEC_G, L.VEC_LB, L.VEC_UB))
            assert G.same_bits(self.x, np.ascontiguousarray(x, self.dt)) and G.same_bits(self.g, np.ascontiguousarray(g, self.dt))
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        if self.h:
            self.core.lbfgsx_destroy(self.h)
            self.h = None

    def up(self, which, a):
        self.L.check(self.core.lbfgsx_upload(self.h, which, _p(np.ascontiguousarray(a, self.dt))))

    def vec(self, which):
        a = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, _p(a)))
        return a

    def cv(self, which):
        a = np.empty(self.n, np.int32 if which == G.CV_VALS_OUT else self.dt)
        self.L.check(self.core.lbfgsx_b_cauchy_download(self.h, which, _p(a)))
        return a

    def state(self):
        st = np.empty(self.n, np.uint8)
        self.L.check(self.core.lbfgsx_b_download_state(self.h, _p(st)))
        return st

    def build(self, tau=None):
        nf, no, ns, dd = i64(-1), i64(-1), i64(-1), f64(math.nan)
        wtd = np.full(80, np.nan)
        if tau is None:
            self.L.check(self.core.lbfgsx_b_cauchy_build(self.h, C.byref(nf), C.byref(no), C.byref(dd), _p(wtd)))
            ns = no
        else:
            self.L.check(self.core.lbfgsx_b_cauchy_build_partial(self.h, tau, C.byref(nf), C.byref(no), C.byref(ns), C.byref(dd), _p(wtd)))
        return nf.value, no.value, ns.value, dd.value, wtd

    def chunk(self, first, count, idx=True, wrows=True):
        brk, g, z = (np.full(count, np.nan) for _ in range(3))
        ix = np.full(count, -7, np.int32) if idx else None
        w = np.full((count, 2 * self.c), np.nan) if (wrows and self.c) else None
        self.L.check(self.core.lbfgsx_b_cauchy_chunk(self.h, first, count, _p(brk), _p(g), _p(z), _p(ix), _p(w)))
        return dict(brk=brk, g=g, z=z, idx=ix, w=w)

    def scan(self, first, count, nord, Mmat, theta, t_prev, state):
        nc2 = 2 * self.c
        out = np.full(2 * nc2 + 3, np.nan)
        e = i64(-99)
        Mmat = np.ascontiguousarray(Mmat, np.float64)
        state = np.ascontiguousarray(state, np.float64)
        rc = self.core.lbfgsx_b_cauchy_scan(self.h, first, count, nord, _p(Mmat) if Mmat.size else _p(np.zeros(1)), theta, t_prev,
                                            _p(state), C.byref(e), _p(out))
        return rc, e.value, out

    def finish(self, t_cross, tfinal, crossed_all):
        na, nf = i64(-1), i64(-1)
        self.L.check(self.core.lbfgsx_b_cauchy_finish(self.h, t_cross, tfinal, crossed_all, C.byref(na), C.byref(nf)))
        return na.value, nf.value

    # ---- comparisons
    def check_build(self, got, ref, what, cols=None):
        """the vectors of a build bit for bit over all rows, the counts exactly, d.d (and W'd) as correctly rounded sums"""
        nf, no, ns, dd, wtd = got
        for name, a, r in (("x", self.vec(self.L.VEC_X), ref.x), ("brk", self.cv(G.CV_BRK), ref.brk), ("d", self.cv(G.CV_DVEC), ref.d),
                           ("xcp", self.vec(self.L.VEC_XCP), ref.xcp), ("g", self.vec(self.L.VEC_G), self.g),
                           ("lb", self.vec(self.L.VEC_LB), self.lb), ("ub", self.vec(self.L.VEC_UB), self.ub)):
            if not G.same_bits(a, r):
                bad = G.diff_rows(a, r)
                raise AssertionError("%s: %s differs in %d rows, first row %d: got %r, reference %r" % (what, name, bad.size, bad[0], a[bad[0]], r[bad[0]]))
        assert (nf, no) == (ref.nfree, ref.nord), "%s: nfree, nord = %r, reference %r" % (what, (nf, no), (ref.nfree, ref.nord))
        bound = B.sum_bound(self.n, ref.dd_abs, ref.d, ref.d)
        assert B.check_rounded(dd, ref.dd_exact, bound, self.dt) != "wrong", "%s: d.d = %r, correctly rounded %r" % (
            what, dd, B.stored(ref.dd_exact, self.dt))
        if cols is not None and self.c:
            ws = B.wtv_sums(cols, ref.d, np.ones(self.n, bool))
            B.judge(wtd[:2 * self.c], ws.exact, ws.bound, self.dt, 0, what + ": W'd")

    def check_sorted(self, ref, want_rows, what, first=0):
        """sorted positions [first, first + len(want_rows)) read through lbfgsx_b_cauchy_chunk against the reference's list"""
        if want_rows.size == 0:
            return
        ch = self.chunk(first, want_rows.size)
        ga = G.gather(want_rows, ref.brk, ref.x, self.g, ref.d, self.lb, self.ub)
        assert np.array_equal(ch["idx"], ga["idx"]), "%s: the rows of the sorted list differ, first at position %d" % (
            what, first + int(np.nonzero(ch["idx"] != ga["idx"])[0][0]))
        for k in ("brk", "g", "z"):
            assert G.same_bits(ch[k], ga[k]), "%s: %s of the sorted list differs at positions %s" % (what, k, G.diff_rows(ch[k], ga[k])[:8])


def _edge_ctx(lib, dt, n, seed, force=False, pairs=(), m=None):
    r = G.edge_rows(n, dt, seed)
    cx = Ctx(lib, dt, r["x_out"] if force else r["x"], r["g"], r["lb"], r["ub"], pairs, m)
    return cx, r


def _plain_rows(n, dt, seed):
    """interior rows with distinct break points (with overwhelming probability; asserted where it matters)"""
    rng = np.random.default_rng([seed, n, 47])
    T = np.dtype(dt).type
    lb, ub = (-1.0 - rng.random(n)).astype(T), (1.0 + rng.random(n)).astype(T)
    x = (0.9 * (2 * rng.random(n) - 1)).astype(T)
    g = rng.standard_normal(n).astype(T)
    g[g == 0] = T(1)
    return x, g, lb, ub


def _distinct_rows(n, dt, seed):
    """rows whose break points are n distinct numbers (i + 1) / 16384 in scattered order: x = t g with g a power of two, the
    bound that is met at 0"""
    assert n < 16384
    rng = np.random.default_rng([seed, n, 53])
    T = np.dtype(dt).type
    t = (1.0 + rng.permutation(n)) / 16384.0
    sc = np.array([1.0, 2.0, 0.5, 4.0])[rng.integers(0, 4, n)]
    neg = rng.random(n) < 0.5
    g = np.where(neg, -sc, sc)
    return (t * g).astype(T), g.astype(T), np.where(neg, -1e6, 0.0).astype(T), np.where(neg, 0.0, 1e6).astype(T)


# ---------------------------------------------------------------- build
@pytest.mark.parametrize("dt,n", [(dt, n) for dt in DTYPES for n in _row_counts(dt)], ids=_ids)
def test_build_rows(lib, dt, n):
    for force in (False, True):
        cx, r = _edge_ctx(lib, dt, n, 11, force)
        with cx:
            if force:
                cx.L.check(cx.core.lbfgsx_b_force_bounds_deferred(cx.h))
            ref = G.build(cx.x, cx.g, cx.lb, cx.ub, force)
            if force:
                assert ref.moved == min(4, max(0, n - 20)) and G.same_bits(ref.x, r["x"])
            got = cx.build()
            cx.check_build(got, ref, "build(force = %s)" % force)
            o = G.order(ref.brk)
            assert o.size == ref.nord
            if n <= 4096:
                cx.check_sorted(ref, o, "full order")
            else:       # the ends and a window in the middle of the long list, and every row number once
                for first, cnt in ((0, 700), (o.size // 2, 700), (o.size - 700, 700)):
                    cx.check_sorted(ref, o[first:first + cnt], "full order", first)
                assert np.array_equal(cx.cv(G.CV_VALS_OUT)[:o.size], o.astype(np.int32)), "the sorted row numbers"


def test_download_entry(lib):
    core, L = lib
    cx, r = _edge_ctx(lib, F64, 300, 12)
    with cx:
        cx.build()
        a = np.empty(300)
        assert core.lbfgsx_b_cauchy_download(cx.h, 3, _p(a)) == E_INVALID and core.lbfgsx_b_cauchy_download(cx.h, -1, _p(a)) == E_INVALID
        assert core.lbfgsx_b_cauchy_download(cx.h, G.CV_BRK, None) == E_INVALID
        assert core.lbfgsx_b_cauchy_download(None, G.CV_BRK, _p(a)) == E_INVALID
    h = vp()
    L.check(core.lbfgsx_create(C.byref(h), L.F64, 300, 3, 0, 0))
    try:
        assert core.lbfgsx_b_cauchy_download(h, G.CV_BRK, _p(a)) == E_INVALID
    finally:
        core.lbfgsx_destroy(h)


# ---------------------------------------------------------------- the full order, the chunks, the W rows
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("c", [0, 1, 4, 5, 10, 20, 40])
def test_full_order(lib, dt, c):
    n = G.EDGE_NEED + 1100
    T = np.dtype(dt).type
    rng = np.random.default_rng([c, 13])
    pairs = [(rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)) for _ in range(c + 3 if c else 0)]
    # pair k lives in slot k % m of the ring, the newest pair wins (BFGSMat.h:101-146); W's columns are in slot order
    kept = [pairs[max(k for k in range(len(pairs)) if k % c == j)] for j in range(c)]
    cols = [p[1] for p in kept] + [p[0] for p in kept]
    cx, r = _edge_ctx(lib, dt, n, 13, pairs=pairs, m=max(c, 1))
    with cx:
        assert cx.c == c
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        cx.check_build(cx.build(), ref, "build", cols)
        o = G.order(ref.brk)
        nord = o.size
        assert nord > 1030
        ga = G.gather(o, ref.brk, ref.x, cx.g, ref.d, cx.lb, cx.ub, cols)
        for first, count in ((0, nord), (3, 1), (nord - 1, 1), (5, 512), (0, 513), (nord - 300, 300)):
            ch = cx.chunk(first, count)
            sl = slice(first, first + count)
            assert np.array_equal(ch["idx"], ga["idx"][sl]), "chunk(%d, %d): rows" % (first, count)
            for k in ("brk", "g", "z") + (("w",) if c else ()):
                assert G.same_bits(ch[k], np.ascontiguousarray(ga[k][sl])), "chunk(%d, %d): %s differs" % (first, count, k)
        # the chunk launched ahead by the partial build: first = 0, count = min(512, nsorted), no idx
        tau = float(ref.brk[o[700]])
        got = cx.build(tau)
        pre = G.prefix(ref.brk, tau)
        assert got[2] == pre.size >= 512
        ch = cx.chunk(0, 512, idx=False)
        for k in ("brk", "g", "z") + (("w",) if c else ()):
            assert G.same_bits(ch[k], np.ascontiguousarray(ga[k][:512])), "chunk ahead: %s differs" % k
        cx.check_sorted(ref, pre, "prefix after the chunk ahead")


# ---------------------------------------------------------------- the partial sort, route by route
def _partial_case(lib, dt, n, seed, counts, what, expect_small=None):
    """first call at a threshold that keeps a handful, then one call per candidate count on the same context"""
    core, L = lib
    x, g, lb, ub = _distinct_rows(n, dt, seed)
    with Ctx(lib, dt, x, g, lb, ub) as cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        o = G.order(ref.brk)
        assert o.size == n > max(counts) and (np.diff(ref.brk[o]) > 0).all()
        taus = [float(ref.brk[o[5]])] + [float(ref.brk[o[k - 1]]) for k in counts]
        for call, tau in enumerate(taus):
            cnt = (i64 * 1)()
            core.lbfgsx_b_psel_counts(cnt, 1)
            got = cx.build(tau)
            core.lbfgsx_b_psel_counts(cnt, 0)
            pre = G.prefix(ref.brk, tau)
            assert pre.size == ([6] + list(counts))[call]
            cx.check_build(got, ref, "%s, call %d" % (what, call))
            assert got[2] == pre.size, "%s, call %d: nsorted %d, %d break points <= tau" % (what, call, got[2], pre.size)
            cx.check_sorted(ref, pre, "%s, call %d" % (what, call))
            if expect_small is not None and call > 0:
                assert cnt[0] == (1 if expect_small(pre.size) else 0), "%s: one-block sort %s at %d candidates" % (
                    what, "missing" if cnt[0] == 0 else "ran", pre.size)
        cx.L.check(core.lbfgsx_b_cauchy_sort_full(cx.h))
        cx.check_sorted(ref, o, what + ": sort_full")


COUNTS = (1, 2, 127, 128, 129, 4095, 4096, 4097)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("route", ["default", "sync_merge0", "psel_small0", "select_inline0", "cap_at", "cap_below"])
def test_partial_routes(lib, dt, route, monkeypatch):
    n = 9001
    small = lambda k: k <= 4096      # noqa: E731
    if route == "default":
        _partial_case(lib, dt, n, 21, COUNTS, route, small)
    elif route == "sync_merge0":
        monkeypatch.setenv("LBFGSX_SYNC_MERGE", "0")
        _partial_case(lib, dt, n, 22, COUNTS, route, small)
    elif route == "psel_small0":
        monkeypatch.setenv("LBFGSX_PSEL_SMALL", "0")
        _partial_case(lib, dt, n, 23, COUNTS, route, lambda k: False)
    elif route == "select_inline0":
        monkeypatch.setenv("LBFGSX_SELECT_INLINE", "0")
        _partial_case(lib, dt, n, 24, (1, 129, 4097), route, lambda k: False)
    elif route == "cap_at":
        monkeypatch.setenv("LBFGSX_SELECT_CAP", "129")
        _partial_case(lib, dt, n, 25, (129, 128), route, small)
    else:
        monkeypatch.setenv("LBFGSX_SELECT_CAP", "128")      # 129 candidates overflow the list: the selection pass takes over
        _partial_case(lib, dt, n, 26, (129, 128, 4097), route, lambda k: k <= 128)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("sync", ["1", "0"])
def test_partial_ties(lib, dt, sync, monkeypatch):
    """thresholds that select the full sort; a threshold ON the break point of the 300-row group keeps the whole group, one
    ulp below none of it; below every break point nothing is sorted -- on the first call's route and on the listed one"""
    monkeypatch.setenv("LBFGSX_SYNC_MERGE", sync)
    core, L = lib
    T = np.dtype(dt).type
    cx, r = _edge_ctx(lib, dt, G.EDGE_NEED + 1500, 27)
    with cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        o = G.order(ref.brk)
        for tau in (0.0, -1.0, math.inf, math.nan):
            got = cx.build(tau)
            cx.check_build(got, ref, "tau = %r" % tau)
            assert got[2] == ref.nord
            cx.check_sorted(ref, o, "tau = %r: full sort" % tau)
        tie = float(ref.brk[r["label"] == "tie5"][0])
        least = float(ref.brk[o[0]])
        assert 0 < least < np.finfo(T).tiny, "the smallest break point is the subnormal one"
        taus = (tie, float(np.nextafter(T(tie), T(0))), float(np.nextafter(T(least), T(0))), tie, float(np.nextafter(T(tie), T(0))), least)
        sizes = []
        for tau in taus:
            got = cx.build(tau)
            pre = G.prefix(ref.brk, tau)
            cx.check_build(got, ref, "tau = %r" % tau)
            assert got[2] == pre.size, "tau = %r: nsorted %d, reference %d" % (tau, got[2], pre.size)
            cx.check_sorted(ref, pre, "tau = %r" % tau)
            sizes.append(pre.size)
        assert sizes[0] - sizes[1] == 300 and sizes[2] == 0 and sizes[5] == 1
        L.check(core.lbfgsx_b_cauchy_sort_full(cx.h))
        cx.check_sorted(ref, o, "sort_full after nsorted = 1")


# ---------------------------------------------------------------- the blocks' list buffers
@pytest.mark.parametrize("n", [1024 * 3, 1024 * 1024 + 4096 * 70], ids=str)
def test_list_buffers(lib, n):
    """f32, every row a candidate of the listed partial sort: each block's 1024-entry buffer exactly full (n = 1024 B), and
    above the grid cap, where a block meets 1280 rows or more and the direct append takes the overflow"""
    x, g, lb, ub = _plain_rows(n, F32, 31)
    with Ctx(lib, F32, x, g, lb, ub) as cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        o = G.order(ref.brk)
        assert o.size == n
        t_small = float(ref.brk[o[9]])
        assert cx.build(t_small)[2] == G.prefix(ref.brk, t_small).size
        # the call before kept 10 <= kPselMax candidates and psel_cap = min(2^21, n) = n, so this build lists its candidates
        # itself (no counter says so for more than 4096 of them: lbfgsx_b_psel_counts counts the one-block sort only)
        got = cx.build(1e30)
        cx.check_build(got, ref, "every row listed")
        assert got[2] == n
        rows = cx.cv(G.CV_VALS_OUT)
        assert np.array_equal(np.sort(rows), np.arange(n, dtype=np.int32)), "a row is lost from, or twice in, the listed candidates"
        assert np.array_equal(rows, o.astype(np.int32)), "the listed candidates' order"
        for first, cnt in ((0, 600), (n // 2, 600), (n - 600, 600)):
            cx.check_sorted(ref, o[first:first + cnt], "every row listed", first)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("cap", ["count", "count-1", "1"])
def test_newact_cap(lib, dt, cap, monkeypatch):
    """the newly active list of k_cauchy_finish on both sides of its capacity, through W_A'(A'd)"""
    n, c = 5003, 3
    rng = np.random.default_rng(33)
    T = np.dtype(dt).type
    x, g, lb, ub = _distinct_rows(n, dt, 33)
    ref0 = G.build(x, g, lb, ub)
    o = G.order(ref0.brk)
    count = 1500
    t_one, t_many = float(ref0.brk[o[0]]), float(ref0.brk[o[count - 1]])
    monkeypatch.setenv("LBFGSX_NEWACT_CAP", {"count": str(count), "count-1": str(count - 1), "1": "1"}[cap])
    pairs = [(rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)) for _ in range(c)]
    cols = [p[1] for p in pairs] + [p[0] for p in pairs]
    with Ctx(lib, dt, x, g, lb, ub, pairs) as cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        cx.build()
        # a search asks for the list when the one before made at most `cap` rows active: none for the first; the second is
        # asked for 1500 after 1 (fits exactly, overflows by one, overflows); the third after 1500 (asked, not asked, not asked)
        for rep, (tc, want) in enumerate(((t_one, 1), (t_many, count), (t_many, count))):
            na, nf = cx.finish(tc, 0.01, 0)
            f = G.finish(ref.brk, ref.x, ref.d, cx.lb, cx.ub, tc, 0.01, 0)
            assert (na, nf) == (f["nact"], f["nfree"]) and na == want
            out, nnz = np.full(2 * c, np.nan), i64(-1)
            cx.L.check(cx.core.lbfgsx_b_wtv(cx.h, VS_DRT, ST_NEWACT, _p(out), C.byref(nnz)))
            rows = f["st"] == G.ST_NEWACT
            ws = B.wtv_sums(cols, f["drt"], rows)
            B.judge(out, ws.exact, ws.bound, cx.dt, 0, "W_A'(A'd), cap %s, search %d" % (cap, rep))
            assert nnz.value == int(np.count_nonzero(f["drt"][rows]))
            assert np.array_equal(cx.state(), f["st"])


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("cap", ["count", "count-1", "1"])
def test_compact_list_cap(lib, dt, cap, monkeypatch):
    """the list of the rows outside the kept compact copy on which d or s_new is not zero (k_cauchy_build's olist), on both
    sides of LBFGSX_WTD_LIST_CAP: W'd and the deferred correction dots are the exact sums either way, and the sums over the
    copy and the list (kx_multidot2_wf) ran exactly when the list fitted.  The state is the solver's: a search that leaves
    4400 of 6000 rows free, the full Gram pass of the first solve with the compaction hint (it writes the copy), a new pair in
    the oldest slot, lbfgsx_b_correction_dots_defer, the next build."""
    core, L = lib
    n, c, nact = 6000, 3, 1600
    T = np.dtype(dt).type
    rng = np.random.default_rng(37)
    x, g, lb, ub = _distinct_rows(n, dt, 37)
    monkeypatch.setenv("LBFGSX_WTD_LIST_CAP", {"count": str(nact), "count-1": str(nact - 1), "1": "1"}[cap])
    pairs = [(rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)) for _ in range(c + 1)]
    with Ctx(lib, dt, x, g, lb, ub, pairs[:c]) as cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        o = G.order(ref.brk)
        cols = [p[1] for p in pairs[:c]] + [p[0] for p in pairs[:c]]
        cx.check_build(cx.build(), ref, "first build", cols)
        tc = float(ref.brk[o[nact - 1]])
        f = G.finish(ref.brk, ref.x, ref.d, cx.lb, cx.ub, tc, 0.01, 0)
        assert cx.finish(tc, 0.01, 0) == (nact, n - nact) == (f["nact"], f["nfree"])
        L.check(core.lbfgsx_b_sub_begin(cx.h))
        L.check(core.lbfgsx_b_set_compaction(cx.h, 1))
        t = 2 * c
        gram, w, gd = np.full((t, t), np.nan), np.full(t, np.nan), np.full(t * (t + 1), np.nan)
        L.check(core.lbfgsx_b_gram_fused_dd(cx.h, G.ST_FREE, VS_DRT, 0, None, None, _p(gram), _p(w), _p(gd)))
        free = f["st"] == G.ST_FREE
        ws = B.wtv_sums(cols, f["drt"], free)
        B.judge(w, ws.exact, ws.bound, F64, 0, "W_F'd of the pass that writes the copy")      # delivered un-rounded, as a double
        # the new pair takes slot 0 (the oldest); its s is not zero on any row, so every row outside the copy is listed
        s_new, y_new = pairs[c]
        L.check(core.lbfgsx_bfgs_add_correction_host(cx.h, _p(s_new), _p(y_new)))
        assert core.lbfgsx_bfgs_ncorr(cx.h) == c and (s_new != 0).all()
        kept = [pairs[3], pairs[1], pairs[2]]
        cols = [p[1] for p in kept] + [p[0] for p in kept]
        outside = int((~free).sum())
        assert outside == nact
        L.check(core.lbfgsx_b_correction_dots_defer(cx.h))
        cnt = (i64 * 4)()
        core.lbfgsx_b_compact_vec_counts(cnt, 1)
        got = cx.build()
        core.lbfgsx_b_compact_vec_counts(cnt, 0)
        cx.check_build(got, ref, "build over the copy and the list, cap %s" % cap, cols)
        assert cnt[2] == (1 if cap == "count" else 0), "cap %s: the pass over the copy and the list %s" % (
            cap, "did not run" if cnt[2] == 0 else "ran on an overflowed list")
        sd, yd = np.full(40, np.nan), np.full(40, np.nan)
        L.check(core.lbfgsx_b_correction_dots(cx.h, _p(sd), _p(yd)))
        cs_ = B.wtv_sums(cols, s_new, np.ones(n, bool))
        B.judge(np.concatenate([yd[:c], sd[:c]]), cs_.exact, cs_.bound, cx.dt, 0, "deferred correction dots, cap %s" % cap)
        cx.check_sorted(ref, o, "the list after the build over the copy")


# ---------------------------------------------------------------- finish
@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("dt,n", [(dt, n) for dt in DTYPES for n in _row_counts(dt)], ids=_ids)
def test_finish_rows(lib, dt, n, fuse, monkeypatch):
    monkeypatch.setenv("LBFGSX_FINISH_FUSE", fuse)
    T = np.dtype(dt).type
    cx, r = _edge_ctx(lib, dt, n, 41)
    with cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        cx.check_build(cx.build(), ref, "build")
        o = G.order(ref.brk)
        big = n > 100000
        has_tie = (r["label"] == "tie5").any()
        tie = float(ref.brk[r["label"] == "tie5"][0]) if has_tie else (float(ref.brk[o[o.size // 2]]) if o.size else 0.5)
        top = float(ref.brk[o[-1]]) if o.size else 1.0
        least = float(ref.brk[o[0]]) if o.size else 1.0
        tcs = [tie, float(np.nextafter(T(tie), T(0))), float(np.nextafter(T(tie), T(np.inf))), 0.0, float(np.nextafter(T(least), T(0))),
               top, 2 * top]
        tfs = [0.0, 0.1, 1.0 / 3.0, tie]
        combos = [(tc, tf, ca) for tc in tcs for tf in tfs for ca in (0, 1)]
        if big:
            combos = [(tcs[0], 0.1, 0), (tcs[1], 1.0 / 3.0, 1), (tcs[2], 0.0, 0)]
        before_d = cx.vec(cx.L.VEC_D)
        for tc, tf, ca in combos:
            na, nf = cx.finish(tc, tf, ca)
            f = G.finish(ref.brk, ref.x, ref.d, cx.lb, cx.ub, tc, tf, ca)
            what = "finish(t_cross = %r, tfinal = %r, crossed_all = %d)" % (tc, tf, ca)
            assert (na, nf) == (f["nact"], f["nfree"]), "%s: nact, nfree = %r, reference %r" % (what, (na, nf), (f["nact"], f["nfree"]))
            xcp, st = cx.vec(cx.L.VEC_XCP), cx.state()
            assert G.same_bits(xcp, f["xcp"]), "%s: xcp differs in rows %s" % (what, G.diff_rows(xcp, f["xcp"])[:8])
            assert np.array_equal(st, f["st"]), "%s: state bytes differ in rows %s" % (what, np.nonzero(st != f["st"])[0][:8])
            d = cx.vec(cx.L.VEC_D)
            want_d = f["drt"] if fuse == "1" else before_d
            assert G.same_bits(d, want_d), "%s: drt differs in rows %s" % (what, G.diff_rows(d, want_d)[:8])
            for name, a, w in (("x", cx.vec(cx.L.VEC_X), ref.x), ("brk", cx.cv(G.CV_BRK), ref.brk), ("d", cx.cv(G.CV_DVEC), ref.d)):
                assert G.same_bits(a, w), "%s: %s changed" % (what, name)
        if has_tie:
            grp = r["label"] == "tie5"
            cx.finish(tcs[0], 0.1, 0)
            assert (cx.state()[grp] == G.ST_NEWACT).all()
            cx.finish(tcs[1], 0.1, 0)
            assert (cx.state()[grp] == G.ST_FREE).all()


# ---------------------------------------------------------------- the pass of the post statements that builds ahead
def _accepted_point(cx, rng, x, g):
    """xp, gp at the start of a line search and the accepted point x, g, placed in the context's buffers"""
    L, n, T = cx.L, cx.n, cx.dt
    xp = (x - T(0.25) * rng.standard_normal(n).astype(T)).astype(T)
    gp = (g - T(0.5) * (x - xp)).astype(T)        # y = g - gp has the sign of s on every row (or is 0): s.y > 0
    cx.up(L.VEC_X, xp)
    cx.up(L.VEC_G, gp)
    L.check(cx.core.lbfgsx_ls_begin(cx.h))
    cx.up(L.VEC_XT, x)
    cx.up(L.VEC_GT, g)
    L.check(cx.core.lbfgsx_ls_end(cx.h, 0))
    return xp, gp


@pytest.mark.parametrize("dt,n", [(dt, n) for dt in DTYPES for n in _row_counts(dt)[:-1] + [G.EDGE_NEED + 700]], ids=_ids)
def test_post_build(lib, dt, n):
    core, L = lib
    T = np.dtype(dt).type
    rng = np.random.default_rng([n, 51])
    cx, r = _edge_ctx(lib, dt, n, 51)
    with cx:
        ref = G.build(cx.x, cx.g, cx.lb, cx.ub)
        o = G.order(ref.brk)
        tau = float(ref.brk[o[min(o.size - 1, 40)]]) if o.size else 0.5
        cx.check_build(cx.build(tau), ref, "first partial build")       # the next call may list its candidates
        for variant in ("taken", "other tau", "x moved", "clamp moves"):
            xp, gp = _accepted_point(cx, rng, r["x_out"] if variant == "clamp moves" else r["x"], r["g"])
            x, g = cx.vec(L.VEC_X), cx.vec(L.VEC_G)
            cnt = (i64 * 2)()
            core.lbfgsx_b_post_build_counts(cnt, 1)
            out = [f64(math.nan) for _ in range(4)]
            L.check(core.lbfgsx_b_post_linesearch_build(cx.h, tau, *[C.byref(v) for v in out]))
            pg, x2, sy, yy = [v.value for v in out]
            what = "post_linesearch_build, " + variant
            s_ref, y_ref = R.sy_ref(x, xp, g, gp)
            assert pg == R.projg_norm_ref(x, g, cx.lb, cx.ub), what + ": projected-gradient norm"
            for got_, a_, b_, nm in ((x2, x, x, "x.x"), (sy, s_ref, y_ref, "s.y"), (yy, y_ref, y_ref, "y.y")):
                ok, msg = R.check_dot(got_, a_, b_, T)
                assert ok, "%s: %s: %s" % (what, nm, msg)
            core.lbfgsx_b_post_build_counts(cnt, 0)
            assert cnt[0] == 1, what + ": the pass did not carry the Cauchy half"
            use_tau = tau
            if variant == "other tau":
                use_tau = float(np.nextafter(T(tau), T(np.inf)))
            elif variant == "x moved":      # one row put on a bound of its own (or a step away where it has none)
                x = x.copy()
                i = n // 2
                cand = [v for v in (cx.lb[i], cx.ub[i], x[i] + T(1)) if np.isfinite(v) and v != x[i] and cx.lb[i] <= v <= cx.ub[i]]
                moved_row = bool(cand)
                if moved_row:
                    x[i] = cand[0]
                cx.up(L.VEC_X, x)
            elif variant == "clamp moves":
                L.check(core.lbfgsx_b_force_bounds_deferred(cx.h))
            refv = G.build(x, g, cx.lb, cx.ub, variant == "clamp moves")
            got = cx.build(use_tau)
            core.lbfgsx_b_post_build_counts(cnt, 0)
            moved = variant == "clamp moves" and refv.moved > 0
            taken = variant == "taken" or (variant == "clamp moves" and not moved)      # (an upload is a refusal whatever it wrote)
            assert cnt[1] == (1 if taken else 0), "%s: hand-over %s" % (what, "refused" if cnt[1] == 0 else "taken")
            cx.check_build(got, refv, what)
            pre = G.prefix(refv.brk, use_tau)
            assert got[2] == pre.size
            cx.check_sorted(refv, pre, what)
            L.check(core.lbfgsx_b_cauchy_sort_full(cx.h))      # after a hand-over the keys were never written: k_keys_from_brk
            cx.check_sorted(refv, G.order(refv.brk), what + ": sort_full")
        # s and y of the last pass, as the driver-statement tests read them: commit the pair, download the history
        assert sy > 0, "the accepted point must have s.y > 0"
        L.check(core.lbfgsx_commit_correction(cx.h))
        Sv, Yv = np.empty(n, T), np.empty(n, T)
        ncorr, ptr, theta = C.c_int(-1), C.c_int(-1), C.c_double(math.nan)
        L.check(core.lbfgsx_bfgs_download_history(cx.h, _p(Sv), _p(Yv), C.byref(ncorr), C.byref(ptr), C.byref(theta)))
        assert ncorr.value == 1
        assert G.same_bits(Sv, s_ref) and G.same_bits(Yv, y_ref), "s, y of the pass"
        assert theta.value == float(T(T(yy) / T(sy))), "theta = y.y / s.y in T (BFGSMat.h:92)"


# ---------------------------------------------------------------- the device search
def _scan_ctx(lib, cs):
    cx = Ctx(lib, cs.dtype.type, cs.x, cs.g, cs.lb, cs.ub, cs.pairs)
    try:
        b, o, ga = cs.lists()
        cx.check_build(cx.build(), b, "build of " + cs.name)
        cx.check_sorted(b, o[:min(o.size, 2000)], "list of " + cs.name)
        return cx, b, o, ga
    except BaseException:
        cx.close()
        raise


def _args(cs, ga, first, count, state=None, t_prev=None):
    nxt = ga["brk"][first + count] if ga["brk"].size > first + count else None
    sl = slice(first, first + count)
    return (ga["brk"][sl], ga["g"][sl], ga["z"][sl], ga["w"][sl], cs.M, cs.theta, cs.state if state is None else state,
            cs.t_prev if t_prev is None else t_prev, nxt)


def _bitwise(cx, cs, ga, first, count, chain, state=None, t_prev=None):
    nord = ga["brk"].size
    a = _args(cs, ga, first, count, state, t_prev)
    rc, e, out = cx.scan(first, count, nord, cs.Mmat(), cs.theta, a[7], a[6])
    assert rc == 0
    em = G.scan_emulate(*a, cs.dtype, chain=chain)
    what = "%s, scan(%d, %d), %s chain" % (cs.name, first, count, chain)
    assert e == (first + em["exit"] if em["exit"] >= 0 else -1), "%s: exit_at %d, reference %d" % (what, e, em["exit"])
    want = np.array([em["f1"], em["f2"], em["brk"]])
    assert G.same_bits(out, want), "%s: [f', f'', brk] = %r, reference %r" % (what, out.tolist(), want.tolist())
    return e, out


@pytest.mark.parametrize("chain", ["host", "scan"])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_scan_no_pairs(lib, dt, chain, monkeypatch):
    """ncorr == 0: the per-crossing terms and the chains are fixed sequences of IEEE operations: bit for bit"""
    if chain == "scan":
        monkeypatch.setenv("LBFGSX_GCP_CHAIN", "scan")
    P2 = 1 << 17
    # no exit anywhere: the state after the last crossing of every count, up to the end of the list
    cs = G.ScanCase("long", dt, 0, P2 + 1, -1, 61, extra=0, gap=1e-6)
    cx, b, o, ga = _scan_ctx(lib, cs)
    with cx:
        assert o.size == P2 + 1
        for count in (1, 2, 63, 64, 65, 255, 256, 257, 513, 64 * 256 + 1, P2 - 1, P2, P2 + 1):
            e, _ = _bitwise(cx, cs, ga, 0, count, chain)
            assert e == -1
        _bitwise(cx, cs, ga, P2 - 700, 701, chain, t_prev=float(ga["brk"][P2 - 701]))       # first > 0, ends at the end of the list
    # the exit on a boundary of the eight pieces of 2^17 crossings, one before and one after
    for ex in (P2 // 8 - 1, P2 // 8, P2 // 8 + 1):
        cs = G.ScanCase("piece%d" % ex, dt, 0, P2, ex, 62, extra=3, gap=1e-6)
        cx, b, o, ga = _scan_ctx(lib, cs)
        with cx:
            e, _ = _bitwise(cx, cs, ga, 0, P2, chain)
            assert e == ex
    # the small placements: crossing 0, the last of a tile, the first of the next, the end of a 300-row group of ties
    for name, count, ex, tie in (("e0", 300, 0, None), ("e255", 600, 255, None), ("e256", 600, 256, None), ("tie", 600, 399, (100, 300))):
        cs = G.ScanCase(name, dt, 0, count, ex, 63, tie=tie, extra=4)
        cx, b, o, ga = _scan_ctx(lib, cs)
        with cx:
            e, _ = _bitwise(cx, cs, ga, 0, count, chain)
            assert e == ex
            if tie:
                assert (np.diff(ga["brk"][100:400]) == 0).all() and (np.diff(ga["idx"][100:400]) > 0).all()


_CASES = G.scan_cases()


@pytest.mark.parametrize("chain", ["host", "scan"])
@pytest.mark.parametrize("cs", _CASES, ids=lambda c: c.name)
def test_scan_pairs(lib, cs, chain, monkeypatch):
    """ncorr > 0: the exit index is the exact search's, p, c, f', f'' lie within scan_bound of it"""
    if chain == "scan":
        monkeypatch.setenv("LBFGSX_GCP_CHAIN", "scan")
    cx, b, o, ga = _scan_ctx(lib, cs)
    with cx:
        nc2 = 2 * cs.c
        a = _args(cs, ga, 0, cs.count)
        ex = G.search_exact(*a)
        upto = ex["exit"] if ex["exit"] >= 0 else cs.count - 1
        bd = G.scan_bound(*a, cs.dtype, ex, upto, chain=chain)
        rc, e, out = cx.scan(0, cs.count, o.size, cs.Mmat(), cs.theta, cs.t_prev, cs.state)
        assert rc == 0
        assert e == ex["exit"], "%s: exit_at %d, exact search %d" % (cs.name, e, ex["exit"])
        assert out[2 * nc2 + 2] == ga["brk"][upto]
        worst = 0.0
        for j in range(nc2):
            for nm, got, want, bnd in (("p", out[j], ex["p"][upto][j], bd["p"][j]), ("c", out[nc2 + j], ex["c"][upto][j], bd["c"][j])):
                err = abs(Fraction(float(got)) - want)
                worst = max(worst, float(err) / bnd if bnd else 0.0)
                assert err <= bnd, "%s: %s[%d] = %r is off the exact %r by %.3g, bound %.3g" % (cs.name, nm, j, got, float(want), float(err), bnd)
        for nm, got, want, bnd in (("f'", out[2 * nc2], ex["f1"][upto], bd["f1"]), ("f''", out[2 * nc2 + 1], ex["f2"][upto], bd["f2"])):
            err = abs(Fraction(float(got)) - want)
            worst = max(worst, float(err) / bnd)
            assert err <= bnd, "%s: %s = %r is off the exact %r by %.3g, bound %.3g" % (cs.name, nm, got, float(want), float(err), bnd)
        print("%s %s: largest error / bound = %.3g" % (cs.name, chain, worst))


@pytest.mark.parametrize("chain", ["host", "scan"])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_scan_two_calls(lib, dt, chain, monkeypatch):
    """a search continued in a second call (first > 0, t_prev and state_in from the first): without pairs bit for bit the
    emulation of the same two calls, and the exit of the exact search over the whole range; with pairs that exit"""
    if chain == "scan":
        monkeypatch.setenv("LBFGSX_GCP_CHAIN", "scan")
    for c in (0, 2):
        cs = G.ScanCase("two", dt, c, 700, 650, 71, extra=4)
        cx, b, o, ga = _scan_ctx(lib, cs)
        with cx:
            nc2 = 2 * c
            whole = G.search_exact(*_args(cs, ga, 0, 700))
            assert whole["exit"] == 650
            if c == 0:
                e1, out1 = _bitwise(cx, cs, ga, 0, 300, chain)
                assert e1 == -1
                e2, _ = _bitwise(cx, cs, ga, 300, 400, chain, state=out1[:2], t_prev=float(out1[2]))
            else:
                rc, e1, out1 = cx.scan(0, 300, o.size, cs.Mmat(), cs.theta, 0.0, cs.state)
                assert rc == 0 and e1 == -1 and out1[2 * nc2 + 2] == ga["brk"][299]
                rc, e2, out2 = cx.scan(300, 400, o.size, cs.Mmat(), cs.theta, float(out1[2 * nc2 + 2]), out1[:2 * nc2 + 2])
                assert rc == 0 and out2[2 * nc2 + 2] == ga["brk"][650]
                bd = G.scan_bound(*_args(cs, ga, 0, 700), cs.dtype, whole, 650, chain=chain, calls=2)
                want = whole["p"][650] + whole["c"][650] + [whole["f1"][650], whole["f2"][650]]
                bnds = list(bd["p"]) + list(bd["c"]) + [bd["f1"], bd["f2"]]
                for j, (wv, bv) in enumerate(zip(want, bnds)):
                    err = abs(Fraction(float(out2[j])) - wv)
                    assert err <= bv, "two calls: state[%d] = %r is off the exact %r by %.3g, bound %.3g" % (j, out2[j], float(wv), float(err), bv)
            assert e2 == 650


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_scan_refusals(lib, dt):
    cs = G.ScanCase("ref", dt, 2, 300, 100, 72, extra=4)
    cx, b, o, ga = _scan_ctx(lib, cs)
    with cx:
        nord = o.size
        good = cx.scan(0, 300, nord, cs.Mmat(), cs.theta, 0.0, cs.state)
        assert good[0] == 0 and good[1] == 100
        for first, count, no in ((0, 0, nord), (0, -1, nord), (-1, 10, nord), (nord - 5, 6, nord), (0, nord + 1, nord)):
            rc, e, out = cx.scan(first, count, no, cs.Mmat(), cs.theta, 0.0, cs.state)
            assert rc == E_INVALID and e == -99 and np.isnan(out).all(), "scan(%d, %d) must be refused untouched" % (first, count)
        again = cx.scan(0, 300, nord, cs.Mmat(), cs.theta, 0.0, cs.state)
        assert again[1] == good[1] and G.same_bits(again[2], good[2]), "a refused call changed the search's state"
        cx.check_sorted(b, o, "the list after refusals")


# ---------------------------------------------------------------- a whole search
@pytest.mark.parametrize("devmin", ["-1", "0", "7"])
@pytest.mark.parametrize("dt,n", [(dt, n) for dt in DTYPES for n in (1, 2, 3, 63, 64, 65, 257)], ids=_ids)
def test_whole_search(lib, dt, n, devmin, monkeypatch):
    import lbfgspp_amd as A
    import oracle_lib as O
    import test_lbfgsb_gpu as TB
    monkeypatch.setenv("LBFGSX_GCP_DEVICE_MIN", devmin)
    r = G.edge_rows(n, dt, 81, extreme=False)
    want = G.whole_search(r["x"], r["g"], r["lb"], r["ub"], int(devmin))
    if n >= 63:
        assert want["crossings"] > 8 and want["nfree"] > 0, "the search must pass the hand-over point and stop inside the list"
    none = np.zeros((0, n), dt)
    got = TB._device_cauchy_subspace(A, O.F64 if dt == F64 else O.F32, 3, none, none, r["x"], r["g"], r["lb"], r["ub"], subspace=False)
    assert (got["crossings"], got["nact"], got["nfree"]) == (want["crossings"], want["nact"], want["nfree"])
    assert np.array_equal(got["state"], want["st"]), "state bytes differ in rows %s" % np.nonzero(got["state"] != want["st"])[0][:8]
    assert G.same_bits(got["xcp"], want["xcp"]), "xcp differs in rows %s" % G.diff_rows(got["xcp"], want["xcp"])[:8]
