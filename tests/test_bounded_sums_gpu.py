"""-m gpu: the n-length sums of the bounded path against EXACT sums (tests/bounded_sums_ref.py, proved by
tests/test_bounded_sums_ref_cpu.py).  The other Gram tests of the suite compare one device kernel with another; all of them
share DD::add_prod / merge (csrc/reduce.cuh) and most the grid reductions, so a lost `lo`, a dropped tail row, a wrong
logical-to-physical column or an off-by-one of the ballot compaction passes them.  Here every sum is held to the truth:
rounded values to check_rounded (only the correctly rounded value passes outside the derived ambiguity zone), un-rounded
(hi, lo) pairs to check_pair with dd_bound (i8_bound for the integer-MFMA Gram).

Set-up through the ABI only (the sequence of test_selected_entries_and_list_grams_equal_the_full_pass): pairs with
lbfgsx_bfgs_add_correction_host, x0 = 0, lb = -1, ub = 1 and a gradient whose magnitudes are 0, about 0.5 or about 2, so that
lbfgsx_b_cauchy_build, lbfgsx_b_cauchy_finish(1, 1, 0) and lbfgsx_b_sub_begin put every row in ST_FREE or ST_NEWACT at will
(bounded_sums_ref.build_case; magnitudes are drawn around 0.5 and 2 instead of being those two numbers so that v = xcp - x0
is not a three-valued vector).  The state bytes, xcp and d are downloaded and asserted to be what was intended
(D == XCP - X bit for bit); the references use the downloaded mask and vector.

What is asserted per case (check_case), c = pairs stored, T = the context's scalar type:
  lbfgsx_b_cauchy_build     dd = d.d and wtd = W'd against d formed on the host (stores double(T(.)))
  lbfgsx_b_correction_dots  the pass of its own and the deferred route (after lbfgsx_b_correction_dots_defer and a build):
                            the same bits, correctly rounded dots with the newest s
  lbfgsx_b_gram_fused_dd    masks 0 and ST_FREE, vsel -1 and LBFGSX_VS_DRT: gram, wtv (check_rounded, stores in double),
                            gram_dd and lbfgsx_b_gram_last_vrow_dd (check_pair), symmetry, gram == hi + lo;
                            lbfgsx_b_gram_fused and _ex return the same bits
  lbfgsx_b_gram             the blocked k_gram, masks 0 and ST_FREE
  lbfgsx_b_wtv              masks 0, ST_FREE, ST_NEWACT (first call right after the finish: the index list) x
                            LBFGSX_VS_DRT / _LBOUND / _UBOUND, nnz exact
  lbfgsx_b_wtv_prologue, lbfgsx_b_gram_fused_ex with LBFGSX_GP_LINEAR: coef1 NULL (v = -g) and random (numpy restatement)
LBFGSX_GP_RHS: tests/test_subspace_statements_gpu.py (test_gp_rhs), which gives rhs a known value through lbfgsx_b_sub_upload.

Kernel classes by c, from the dispatch code (csrc/lbfgsb_gram.hip gram_dd_core, lbfgsb_dots.hip wtv_t / cauchy_wtd_t,
lbfgsb_x.hip LBFGSX_XCLASS and gram_kpb); default = split-row kernels (LBFGSX_SPLIT=1), 2c columns:
    c   fused Gram, v row (ntot = 2c + 1)   fused Gram, no v     kx_rows / kx_multidot_mask / kx_list1 / kx_multidot2 (NCL, G)
    1   k_gram_dd KP 1  (ntot 3)            k_gram_dd KP 1       (4, 2)
    2   k_gram_dd KP 1  (5)                 KP 1                 (4, 2)
    4   k_gram_dd KP 1  (9)                 KP 1                 (4, 2)
    5   k_gram_dd KP 2  (11)                KP 1                 (6, 2)
    7   k_gram_dd KP 2  (15)                KP 2                 (8, 2)
    8   k_gram_dd KP 4  (17)                KP 4                 (8, 2)
   10   k_gram_dd KP 4  (21)                KP 4                 (10, 2)
   11   k_gram_dd KP 6  (23)                KP 4                 (12, 2)
   13   k_gram_dd KP 6  (27)                KP 6                 (8, 4)
   14   k_gram_dd KP 8  (29)                KP 6                 (8, 4)
   15   k_gram_dd KP 8  (31)                KP 8                 (8, 4)
   16   kx_gram KPB 3   (33)                kx_gram KPB 3 (32)   (8, 4)
   20   kx_gram KPB 4   (41)                kx_gram KPB 4 (40)   (10, 4)
   40   kx_gram KPB 13  (81)                kx_gram KPB 13 (80)  (20, 4)
  lbfgsx_b_gram is k_gram<T, 4> in 4 x 4 column blocks at every c; the deferred correction dots need 2c >= 2 and ride in
  kx_multidot2 of the same (NCL, G).  Blocks: k_gram_dd min(1024, occupancy x CUs, ceil(batches / 4)) of four waves, so the
  row cases 1..257 run in one or two blocks (n = 63, 64, 65: one 64-row batch and its neighbour; 255, 257: the block of 4
  batches), 4095 / 4097 in 16 / 17 blocks, 20011 in 79; 300001 (c = 4) and 70001 (c = 15) make every wave walk several
  batches and take the two-level k_gram_finish (more than 32 partial tiles).
  LBFGSX_SPLIT=0 (test_one_lane_kernels): wtv = k_multidot<8> (2c <= 8), k_multidot_all<16 / 24 / 32>; the v row of
  lbfgsx_b_wtv_prologue = k_vrows<8 / 16 / 20 / 24 / 32, 1>; deferred dots = k_multidot2_all<16 / 20> for 8 < 2c <= 20, the
  separate pass otherwise; ST_NEWACT goes through the mask (no index list).
  LBFGSX_GRAM=i8 (test_integer_gram): k_gram_i8<23> for 2c <= 23, <31> up to 30, masks 0 and ST_FREE; the v row stays
  double-double inside that kernel.  Its bound is relative to the whole column's maximum (i8_bound), so its cases keep
  masked-out rows at the scale of the others; the 2^300 case below is a double-double case only.
  Compact copy (test_compact_copy): with lbfgsx_b_set_compaction(1) and 4096 <= nfree <= 7n/8 the full pass
  (gram_dd != NULL, ST_FREE, a vector selector) writes the compact copy of the free rows and lbfgsx_b_wtv_prologue reads it
  (kx_rows<.., IDX = true>); lbfgsx_counters_ex counts that pass.
  Carried pieces (test_carried_pieces): lbfgsx_b_gram_pairs_dd = kx_rows<.., NA = 3>, lbfgsx_b_gram_list_dd = kx_gram over
  an index list (one block finishes a list of <= 8192 rows itself).

Everything that needs the L / U / P partition (lbfgsx_b_wtv_lu*, lbfgsx_b_solve_sweep*, lbfgsx_b_lu_sweep, lbfgsx_b_wcombine,
lbfgsx_b_solve_wty) and LBFGSX_GP_RHS: tests/test_subspace_statements_gpu.py (the vectors of the subspace minimisation are
observable through lbfgsx_b_sub_download / _sub_upload)."""
import ctypes as C
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import bounded_sums_ref as B
import statement_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
ST_FREE, ST_NEWACT = B.ST_FREE, B.ST_NEWACT
VS_DRT, VS_NEG_CF, VS_LBOUND, VS_UBOUND = 0, 1, 3, 4
GP_NONE, GP_LINEAR = 0, 2
vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double


@pytest.fixture(scope="module")
def lib():
    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1
    pi64, pf64 = C.POINTER(i64), C.POINTER(f64)
    for name, args in (("lbfgsx_b_cauchy_build", [vp, pi64, pi64, pf64, vp]),
                       ("lbfgsx_b_cauchy_finish", [vp, f64, f64, i32, pi64, pi64]),
                       ("lbfgsx_b_sub_begin", [vp]), ("lbfgsx_b_download_state", [vp, vp]),
                       ("lbfgsx_b_gram_fused_dd", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                       ("lbfgsx_b_gram_fused_ex", [vp, i32, i32, i32, vp, vp, vp, vp]),
                       ("lbfgsx_b_gram_fused", [vp, i32, i32, vp, vp]), ("lbfgsx_b_gram", [vp, i32, vp]),
                       ("lbfgsx_b_wtv", [vp, i32, i32, vp, pi64]),
                       ("lbfgsx_b_wtv_prologue", [vp, i32, i32, i32, vp, vp, vp]),
                       ("lbfgsx_b_correction_dots", [vp, vp, vp]), ("lbfgsx_b_correction_dots_defer", [vp]),
                       ("lbfgsx_b_set_compaction", [vp, i32]), ("lbfgsx_b_free_delta", [vp, pi64, pi64]),
                       ("lbfgsx_b_gram_list_dd", [vp, i32, vp]),
                       ("lbfgsx_b_gram_pairs_dd", [vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp])):
        f = getattr(core, name)
        f.restype, f.argtypes = i32, args
    return core, L


def _p(a):
    return a.ctypes.data_as(vp)


class Ctx:
    """one bounded context set up from a built case: history, vectors, Cauchy build / finish / sub_begin"""

    def __init__(self, lib, bt, cols_scale=None):
        self.core, self.L = lib
        core, L = lib
        self.bt, cs = bt, bt.case
        self.dt = np.dtype(cs.dtype).type
        self.n, self.c, self.t = cs.n, bt.c, 2 * bt.c
        self.h = vp()
        L.check(core.lbfgsx_create(C.byref(self.h), L.F64 if cs.dtype == F64 else L.F32, cs.n, cs.m, 0, L.FLAG_BOUNDED))
        self.keep = []
        for s_, y_ in bt.pairs:
            if cols_scale is not None:
                s_, y_ = (s_ * cols_scale).astype(self.dt), (y_ * cols_scale).astype(self.dt)
            self.keep += [s_, y_]
            L.check(core.lbfgsx_bfgs_add_correction_host(self.h, _p(s_), _p(y_)))
        assert core.lbfgsx_bfgs_ncorr(self.h) == self.c

    def close(self):
        if self.h:
            self.core.lbfgsx_destroy(self.h)
            self.h = None

    def upload(self, which, a):
        a = np.ascontiguousarray(a, self.dt)
        self.L.check(self.core.lbfgsx_upload(self.h, which, _p(a)))

    def download(self, which):
        a = np.empty(self.n, self.dt)
        self.L.check(self.core.lbfgsx_download(self.h, which, _p(a)))
        return a

    def vectors(self):
        L, bt = self.L, self.bt
        for which, v in ((L.VEC_X, np.zeros(self.n)), (L.VEC_G, bt.g), (L.VEC_LB, bt.lb), (L.VEC_UB, bt.ub)):
            self.upload(which, v)

    def build(self):
        nf, no, dd = i64(), i64(), f64()
        wtd = np.full(80, np.nan)
        self.L.check(self.core.lbfgsx_b_cauchy_build(self.h, C.byref(nf), C.byref(no), C.byref(dd), _p(wtd)))
        return nf.value, no.value, dd.value, wtd[:self.t].copy()

    def finish(self, tc):
        na, nf = i64(), i64()
        self.L.check(self.core.lbfgsx_b_cauchy_finish(self.h, tc, 1.0, 0, C.byref(na), C.byref(nf)))
        return na.value, nf.value

    def sub_begin(self):
        self.L.check(self.core.lbfgsx_b_sub_begin(self.h))

    def state(self):
        st = np.empty(self.n, np.uint8)
        self.L.check(self.core.lbfgsx_b_download_state(self.h, _p(st)))
        return st

    def corr_dots(self):
        sd, yd = np.full(40, np.nan), np.full(40, np.nan)
        self.L.check(self.core.lbfgsx_b_correction_dots(self.h, _p(sd), _p(yd)))
        return np.concatenate([yd[:self.c], sd[:self.c]])   # logical order [Y slots, S slots]

    def fused_dd(self, mask, vsel, prologue=GP_NONE, coef1=None, dd=True):
        t = self.t
        G, w, gd = np.full((t, t), np.nan), np.full(t, np.nan), np.full(t * (t + 1), np.nan)
        c1 = None if coef1 is None else _p(coef1)
        self.L.check(self.core.lbfgsx_b_gram_fused_dd(self.h, mask, vsel, prologue, c1, None, _p(G), _p(w) if vsel >= 0 else None,
                                                      _p(gd) if dd else None))
        return G, w, gd.reshape(-1, 2)

    def fused_ex(self, mask, vsel, prologue=GP_NONE, coef1=None):
        t = self.t
        G, w = np.full((t, t), np.nan), np.full(t, np.nan)
        c1 = None if coef1 is None else _p(coef1)
        self.L.check(self.core.lbfgsx_b_gram_fused_ex(self.h, mask, vsel, prologue, c1, None, _p(G), _p(w) if vsel >= 0 else None))
        return G, w

    def fused(self, mask, vsel):
        t = self.t
        G, w = np.full((t, t), np.nan), np.full(t, np.nan)
        self.L.check(self.core.lbfgsx_b_gram_fused(self.h, mask, vsel, _p(G), _p(w) if vsel >= 0 else None))
        return G, w

    def vrow_dd(self):
        o = np.full(2 * self.t, np.nan)
        self.L.check(self.core.lbfgsx_b_gram_last_vrow_dd(self.h, o.ctypes.data_as(C.POINTER(f64))))
        return o.reshape(-1, 2)

    def gram(self, mask):
        G = np.full((self.t, self.t), np.nan)
        self.L.check(self.core.lbfgsx_b_gram(self.h, mask, _p(G)))
        return G

    def wtv(self, vsel, mask):
        o, nnz = np.full(self.t, np.nan), i64(-1)
        self.L.check(self.core.lbfgsx_b_wtv(self.h, vsel, mask, _p(o), C.byref(nnz)))
        return o, nnz.value

    def wtv_pro(self, mask, vsel, prologue=GP_NONE, coef1=None):
        o = np.full(self.t, np.nan)
        c1 = None if coef1 is None else _p(coef1)
        self.L.check(self.core.lbfgsx_b_wtv_prologue(self.h, mask, vsel, prologue, c1, None, _p(o)))
        return o


def _tri(G):
    t = G.shape[0]
    return [G[i, j] for i in range(t) for j in range(i + 1)]


def _same_bits(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _pairs(gd, sums, what):
    for e, (ex, bd) in enumerate(zip(sums.exact, sums.bound)):
        B.check_pair(gd[e, 0], gd[e, 1], ex, bd, "%s[%d]" % (what, e))


def _cmax(cx):
    """max |column| over all rows of every logical column, as the i8 kernel's colmax holds it"""
    return [float(np.abs(col).max()) for col in cx.up_cols]


def check_case(lib, cs, i8=False, only_free=False, scale_masked_out=None, bound_selectors=True):
    """every entry of the module docstring on one case; returns the context's outputs of the ST_FREE full pass"""
    core, L = lib
    bt = B.built(cs)
    dt, fam, wid = np.dtype(cs.dtype).type, cs.family, B.case_id(cs)
    scale = None
    if scale_masked_out is not None:
        scale = np.where(bt.free, 1.0, scale_masked_out)
    cx = Ctx(lib, bt, scale)
    cx.up_cols = bt.cols if scale is None else [(col * scale).astype(dt) for col in bt.cols]
    try:
        c, t, n = cx.c, cx.t, cx.n
        allrows = None
        # ---- the dots of add_correction, the pass of its own (v = the newest s, every row)
        s_new = cx.up_cols[c + (cs.npairs - 1) % cs.m]
        if not only_free:
            corr = B.wtv_sums(cx.up_cols, s_new, allrows)
            own = cx.corr_dots()
            B.judge(own, corr.exact, corr.bound, dt, B.cap_for(fam, t), wid + " correction_dots")
        # ---- Cauchy build: d.d and W'd
        cx.vectors()
        nfree0, nord, dd, wtd = cx.build()
        assert nfree0 == int(((bt.kind == B.K_FREE0) | (bt.kind == B.K_INF)).sum())
        assert nord == int(((bt.kind == B.K_FREE) | (bt.kind == B.K_NEWACT)).sum())
        if not only_free:
            exdd = R.exact_dot(bt.dvec, bt.dvec)
            B.judge([dd], [exdd], [B.sum_bound(n, exdd, bt.dvec, bt.dvec)], dt, 0, wid + " d.d")
            wd = B.wtv_sums(cx.up_cols, bt.dvec, allrows)
            B.judge(wtd, wd.exact, wd.bound, dt, B.cap_for(fam, t), wid + " wtd")
            # the deferred route: the next build's W'd pass takes the dots along; same bits on both routes, and the same W'd
            L.check(core.lbfgsx_b_correction_dots_defer(cx.h))
            _, _, dd2, wtd2 = cx.build()
            deferred = cx.corr_dots()
            assert _same_bits(deferred, own) and _same_bits(wtd2, wtd) and dd2 == dd
        # ---- the free and newly active sets
        nact, nfree = cx.finish(1.0)
        assert (nact, nfree) == (int(bt.newact.sum()), int(bt.free.sum()))
        nact, nfree = cx.finish(1.0)      # the second search of a context lists its newly active rows
        assert (nact, nfree) == (int(bt.newact.sum()), int(bt.free.sum()))
        cx.sub_begin()
        na_first = cx.wtv(VS_DRT, ST_NEWACT) if not only_free else None   # right after the finish: the index list
        st = cx.state()
        assert np.array_equal(st, bt.state), "state bytes differ from the intended sets in %d rows" % int((st != bt.state).sum())
        D, XCP, X = cx.download(L.VEC_D), cx.download(L.VEC_XCP), cx.download(L.VEC_X)
        assert np.array_equal(XCP, bt.xcp) and not X.any()
        assert _same_bits((XCP - X).astype(F64), D.astype(F64)) and np.array_equal(D, bt.drt)
        free = (st & ST_FREE) != 0
        newact = (st & ST_NEWACT) != 0
        v = D
        use_i8 = i8 and cs.dtype == F64 and t <= 30
        cmax = _cmax(cx) if use_i8 else None
        out = {}
        # ---- the one-pass Gram
        for mask in ((ST_FREE,) if only_free else (0, ST_FREE)):
            rows = None if mask == 0 else free
            if scale is None:
                gs, ws = B.case_sums(cs, mask)
            else:
                gs, ws = B.gram_sums(cx.up_cols, rows), B.wtv_sums(cx.up_cols, v, rows)
            gsb = B.gram_sums(cx.up_cols, rows, cmax) if use_i8 else gs   # the integer kernel's own bound
            tag = "%s mask %d" % (wid, mask)
            cap = B.cap_for(fam, len(gs.exact) + t)
            for vsel in (-1, VS_DRT):
                G, w, gd = cx.fused_dd(mask, vsel)
                assert np.array_equal(G, G.T), tag + ": gram is not symmetric"
                amb = B.judge(_tri(G), gs.exact, gsb.bound, F64, cap, tag + " gram")
                _pairs(gd, gsb, tag + " gram_dd")
                assert _same_bits(_tri(G), gd[:, 0] + gd[:, 1]), tag + ": gram is not the rounding of its own (hi, lo)"
                if vsel >= 0:
                    B.judge(w, ws.exact, ws.bound, F64, cap - amb, tag + " wtv")
                    vr = cx.vrow_dd()
                    _pairs(vr, ws, tag + " vrow_dd")
                    assert _same_bits(w, vr[:, 0] + vr[:, 1])
                    out[mask] = (G, w, gd)
                Gx, wx = cx.fused_ex(mask, vsel)
                Gf, wf = cx.fused(mask, vsel)
                assert _same_bits(Gx, G) and _same_bits(Gf, G)
                if vsel >= 0:
                    assert _same_bits(wx, w) and _same_bits(wf, w)
            # ---- the blocked Gram (stores double(T(.)))
            B.judge(_tri(cx.gram(mask)), gs.exact, gs.bound, dt, cap, tag + " blocked gram")
        # ---- masked multi-dots
        for mask in ((ST_FREE,) if only_free else (0, ST_FREE, ST_NEWACT)):
            rows = None if mask == 0 else free if mask == ST_FREE else newact
            nr = n if rows is None else int(rows.sum())
            sels = [(VS_DRT, v, True)]
            if bound_selectors:
                sels += [(VS_LBOUND, bt.lb - X, False), (VS_UBOUND, bt.ub - X, False)]
            for vsel, vec, follows_base in sels:
                ws = B.wtv_sums(cx.up_cols, vec, rows)
                got, nnz = cx.wtv(vsel, mask)
                tag = "%s wtv(vsel %d, mask %d)" % (wid, vsel, mask)
                if nr == 0:
                    assert _same_bits(got, np.zeros(t)), tag + ": the empty sum is +0.0"
                B.judge(got, ws.exact, ws.bound, dt, B.cap_for(fam, t, follows_base), tag)
                assert nnz == int(np.count_nonzero(vec if rows is None else vec[rows])), tag + ": nnz"
                if mask == ST_NEWACT and vsel == VS_DRT and na_first is not None:
                    assert _same_bits(na_first[0], got) and na_first[1] == nnz   # index list == state-byte mask
        # ---- the prologue LBFGSX_GP_LINEAR: v = -cF, cF = -1 * (W coef1) + g on the rows of the mask
        rng = np.random.default_rng([cs.seed, 99])
        coef = 0.1 * rng.standard_normal(t)
        for mask in ((ST_FREE,) if only_free else (ST_FREE, 0)):
            rows = None if mask == 0 else free
            for cf in (None, coef):
                _, vref = B.gp_linear_ref(cx.up_cols, cf, bt.g, dt)
                if cf is None:
                    assert np.array_equal(vref, -bt.g)
                ws = B.wtv_sums(cx.up_cols, vref, rows)
                tag = "%s GP_LINEAR(mask %d, coef %s)" % (wid, mask, "NULL" if cf is None else "random")
                cap = B.cap_for(fam, t, cf is None)
                got = cx.wtv_pro(mask, VS_NEG_CF, GP_LINEAR, cf)
                B.judge(got, ws.exact, ws.bound, F64, cap, tag + " wtv_prologue")
                if mask == ST_FREE:
                    G, w = cx.fused_ex(mask, VS_NEG_CF, GP_LINEAR, cf)
                    B.judge(w, ws.exact, ws.bound, F64, cap, tag + " gram_fused_ex")
                    assert _same_bits(G, out[ST_FREE][0]) and _same_bits(got, w)
        return out
    finally:
        cx.close()


# ---------------------------------------------------------------- rows, history lengths, ring wrap, masks
@pytest.mark.parametrize("cs", B.ROW_CASES + B.LONG_CASES, ids=B.case_id)
def test_row_counts(lib, cs):
    """around the 64-row batch, the block of four batches and the 4096-row threshold; the two long cases make every wave
    walk many batches and take the two-level grid reduction"""
    check_case(lib, cs)


@pytest.mark.parametrize("cs", B.HISTORY_CASES, ids=B.case_id)
def test_history_lengths(lib, cs):
    """every pairs-per-lane class of k_gram_dd, the block-tile kx_gram beyond 31 columns, every column-per-lane class of
    the split-row kernels (module docstring)"""
    check_case(lib, cs)


@pytest.mark.parametrize("cs", B.WRAP_CASES, ids=B.case_id)
def test_ring_wrap(lib, cs):
    """m + 3 pairs: storage slots 0..2 hold the three newest pairs, and no slot sits in the physical column of its number"""
    check_case(lib, cs)


@pytest.mark.parametrize("cs", B.MASK_CASES, ids=B.case_id)
def test_masks(lib, cs):
    """every row in, no row in (exact +0.0, asserted bit for bit inside check_case through the exact sum 0), exactly one row
    in at 0, 63, 64 and n - 1, and rows with infinite bounds (free whatever their gradient; no bound selectors there:
    lb - x0 is not finite)"""
    out = check_case(lib, cs, bound_selectors=cs.mask != "rand60inf")
    if cs.mask == "none":
        G, w, gd = out[ST_FREE]
        assert _same_bits(G, np.zeros_like(G)) and _same_bits(w, np.zeros_like(w)) and _same_bits(gd, np.zeros_like(gd))


def test_masked_out_rows_of_magnitude_2_300_change_nothing(lib):
    """double-double kernels only: the rows outside the free set hold finite values near 2^300; every sum over ST_FREE must
    be what it is without them (a kernel that multiplies before it masks would overflow or lose every small term)"""
    big = check_case(lib, B.HUGE_CASE, only_free=True, scale_masked_out=2.0 ** 300)
    plain = check_case(lib, B.HUGE_CASE, only_free=True)
    for a, b in zip(big[ST_FREE], plain[ST_FREE]):
        assert _same_bits(a, b)


@pytest.mark.parametrize("cs", B.FAMILY_CASES, ids=B.case_id)
def test_families(lib, cs):
    """rows spread over twelve decades, and independent columns (condition ~ sqrt(n)): (hi, lo) to check_pair, the rounded
    values to check_rounded under the ambiguity cap"""
    check_case(lib, cs)


@pytest.mark.parametrize("cs", B.F32_CASES, ids=B.case_id)
def test_f32_contexts(lib, cs):
    """D1 accumulators; the one-pass Gram stores doubles, the multi-dots double(float(.)): two roundings"""
    check_case(lib, cs)


# ---------------------------------------------------------------- variants of the same matrices
@pytest.mark.parametrize("cs", B.NOSPLIT_CASES, ids=B.case_id)
def test_one_lane_kernels(lib, monkeypatch, cs):
    monkeypatch.setenv("LBFGSX_SPLIT", "0")
    check_case(lib, cs)


@pytest.mark.parametrize("cs", B.I8_CASES, ids=B.case_id)
def test_integer_gram(lib, monkeypatch, cs):
    """LBFGSX_GRAM=i8: the rounded entries to check_rounded and the un-rounded pairs to check_pair with i8_bound; the same
    bits as the double-double kernel on the same input"""
    monkeypatch.setenv("LBFGSX_GRAM", "i8")
    i8 = check_case(lib, cs, i8=True)
    monkeypatch.setenv("LBFGSX_GRAM", "dd")
    dd = check_case(lib, cs)
    for mask in (0, ST_FREE):
        assert _same_bits(i8[mask][0], dd[mask][0]) and _same_bits(i8[mask][1], dd[mask][1])


def test_integer_gram_past_its_flush_interval(lib, monkeypatch):
    """A wave of k_gram_i8 flushes its int32 accumulators after kI8FlushBatches = 120 batches of 64 rows; the launch has
    min(CUs, ceil(batches / 4)) blocks of four waves, so on 256 CUs n = 8 000 003 gives every wave 122 batches.  c = 1:
    three Gram entries and the v row against exact sums, and bit-identity with the double-double kernel."""
    import torch
    core, L = lib
    cs = B.I8_FLUSH_CASE
    n = cs.n
    t0 = time.time()
    bt = B.built(cs)
    v = bt.drt
    res = {}
    for mode in ("i8", "dd"):
        monkeypatch.setenv("LBFGSX_GRAM", mode)
        cx = Ctx(lib, bt)
        try:
            if mode == "i8":
                cus = torch.cuda.get_device_properties(core.lbfgsx_device(cx.h)).multi_processor_count
                nbatch = (n + 63) // 64
                waves = 4 * min(cus, (nbatch + 3) // 4)
                if nbatch <= 120 * waves:
                    pytest.skip("%d CUs: %d batches over %d waves do not reach the flush after 120" % (cus, nbatch, waves))
            cx.upload(L.VEC_D, v)
            res[mode] = cx.fused_dd(0, VS_DRT)
        finally:
            cx.close()
    gs, ws = B.case_sums(cs, 0)
    cmax = [float(np.abs(col).max()) for col in bt.cols]
    gi8 = B.gram_sums(bt.cols, None, cmax)
    G, w, gd = res["i8"]
    B.judge(_tri(G), gs.exact, gi8.bound, F64, 0, "i8 gram")
    _pairs(gd, gi8, "i8 gram_dd")
    B.judge(w, ws.exact, ws.bound, F64, 0, "i8 wtv")
    Gd, wd, gdd = res["dd"]
    B.judge(_tri(Gd), gs.exact, gs.bound, F64, 0, "dd gram")
    _pairs(gdd, gs, "dd gram_dd")
    assert _same_bits(G, Gd) and _same_bits(w, wd)
    print("8e6-row case: %.1f s" % (time.time() - t0))


# ---------------------------------------------------------------- the compact copy and the carried pieces
@pytest.mark.parametrize("cs", B.COMPACT_CASES, ids=B.case_id)
def test_compact_copy(lib, cs):
    """4096 <= nfree <= 7n/8 after lbfgsx_b_set_compaction(1): the full pass writes the compact copy of the free rows, the
    following lbfgsx_b_wtv_prologue reads it; both against exact sums"""
    core, L = lib
    bt = B.built(cs)
    cx = Ctx(lib, bt)
    cx.up_cols = bt.cols
    try:
        cx.vectors()
        cx.build()
        nact, nfree = cx.finish(1.0)
        assert 4096 <= nfree <= 7 * cs.n // 8
        cx.sub_begin()
        L.check(core.lbfgsx_b_set_compaction(cx.h, 1))
        gs, ws = B.case_sums(cs, ST_FREE)
        G, w, gd = cx.fused_dd(ST_FREE, VS_DRT)               # writes the copy
        B.judge(_tri(G), gs.exact, gs.bound, F64, 0, "gram")
        _pairs(gd, gs, "gram_dd")
        B.judge(w, ws.exact, ws.bound, F64, 0, "wtv")
        cnt = (i64 * 8)()
        L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
        before = (cnt[4], cnt[5])
        got = cx.wtv_pro(ST_FREE, VS_DRT)                       # reads it
        L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
        assert (cnt[4] - before[0], cnt[5] - before[1]) == (1, nfree), "the pass did not walk the compact copy"
        B.judge(got, ws.exact, ws.bound, F64, 0, "wtv_prologue over the copy")
        assert _same_bits(got, w)
        rng = np.random.default_rng(5)
        coef = 0.1 * rng.standard_normal(cx.t)
        _, vref = B.gp_linear_ref(bt.cols, coef, bt.g, cx.dt)
        wl = B.wtv_sums(bt.cols, vref, bt.free)
        L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
        before = cnt[4]
        got = cx.wtv_pro(ST_FREE, VS_NEG_CF, GP_LINEAR, coef)
        L.check(core.lbfgsx_counters_ex(C.byref(cnt), 0))
        assert cnt[4] - before == 1
        B.judge(got, wl.exact, wl.bound, F64, B.cap_for(cs.family, cx.t, False), "GP_LINEAR over the copy")
        G2, w2, gd2 = cx.fused_dd(ST_FREE, VS_DRT)             # the full pass now reads the copy too: another order of the
        assert _same_bits(G2, G) and _same_bits(w2, w)         # additions, the same rounded sums
        _pairs(gd2, gs, "gram_dd over the copy")
    finally:
        cx.close()


@pytest.mark.parametrize("cs", B.CARRIED_CASES, ids=B.case_id)
def test_carried_pieces(lib, cs):
    """lbfgsx_b_gram_pairs_dd (the v row and the rows of two columns) and lbfgsx_b_gram_list_dd (the rows that entered the
    free set) against exact sums directly, not against the full pass"""
    core, L = lib
    bt = B.built(cs)
    cx = Ctx(lib, bt)
    try:
        cx.vectors()
        cx.build()
        c, t = cx.c, cx.t
        nact, nfree = cx.finish(1.0)
        cx.sub_begin()
        ne, nl = i64(), i64()
        L.check(core.lbfgsx_b_free_delta(cx.h, C.byref(ne), C.byref(nl)))
        assert nl.value == 0 and ne.value in (nfree, -1)
        v = cx.download(L.VEC_D)
        assert np.array_equal(v, bt.drt)
        ds = c // 2
        pi, pj = [], []
        for J in range(t):
            pi.append(max(ds, J)); pj.append(min(ds, J))
        for J in range(t):
            if J != ds:
                pi.append(max(c + ds, J)); pj.append(min(c + ds, J))
        for J in range(t + 1):
            pi.append(t); pj.append(J)
        assert len(pi) <= core.lbfgsx_b_gram_pairs_max(cx.h)
        api, apj = (i32 * len(pi))(*pi), (i32 * len(pi))(*pj)
        pd = np.full(2 * len(pi), np.nan)
        L.check(core.lbfgsx_b_gram_pairs_dd(cx.h, ST_FREE, VS_DRT, GP_NONE, None, None, len(pi), api, apj, -2, _p(pd)))
        allc = list(bt.cols) + [v]
        full = B.gram_sums(allc, bt.free)          # (2c + 1) x (2c + 1), the v row and v.v included
        for z, (I, J) in enumerate(zip(pi, pj)):
            e = I * (I + 1) // 2 + J
            B.check_pair(pd[2 * z], pd[2 * z + 1], full.exact[e], full.bound[e], "pairs_dd (%d, %d)" % (I, J))
            assert B.check_rounded(pd[2 * z] + pd[2 * z + 1], full.exact[e], full.bound[e], F64) == "ok"
        # a few more rows free: the newly active rows whose break point lies beyond 0.66 enter
        dt = cx.dt
        with np.errstate(divide="ignore", invalid="ignore"):
            brk = np.where(bt.g < 0, (dt(0) - bt.ub) / bt.g, np.where(bt.g > 0, (dt(0) - bt.lb) / bt.g, dt(np.inf)))
        entered = bt.newact & (brk > dt(0.66))
        assert 10 <= entered.sum() <= 4000
        nact2, nfree2 = cx.finish(0.66)
        assert nfree2 == nfree + int(entered.sum())
        cx.sub_begin()
        L.check(core.lbfgsx_b_free_delta(cx.h, C.byref(ne), C.byref(nl)))
        assert (ne.value, nl.value) == (int(entered.sum()), 0)
        ldd = np.full(t * (t + 1), np.nan)
        L.check(core.lbfgsx_b_gram_list_dd(cx.h, 0, _p(ldd)))
        ldd = ldd.reshape(-1, 2)
        lst = B.gram_sums(bt.cols, entered)
        _pairs(ldd, lst, "list_dd")
        B.judge(ldd[:, 0] + ldd[:, 1], lst.exact, lst.bound, F64, 0, "list_dd rounded")
    finally:
        cx.close()
