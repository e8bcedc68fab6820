"""CPU suite: the criteria of tests/bounded_sums_ref.py are proved here before tests/test_bounded_sums_gpu.py relies on them.
`nearest` against math.fsum and constructed ties; check_rounded / check_pair against mutations of a correct host-side
double-double sum (each a defect the device-against-device comparisons of the suite cannot see); the prologue restatement
against a plain loop; and, for every case the GPU file runs, the precondition that makes "correctly rounded" decidable:
how many exact sums lie within their error bound of a rounding boundary."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bounded_sums_ref as B
import statement_ref as R

F64, F32 = np.float64, np.float32


def _frac_dot(a, b):
    s = Fraction(0)
    for p, q in zip(a, b):
        s += Fraction(float(p)) * Fraction(float(q))
    return s


# ---------------------------------------------------------------- nearest
@pytest.mark.parametrize("n", [1, 2, 33, 1000])
def test_nearest_agrees_with_fsum_on_random_data(n):
    rng = np.random.default_rng(n)
    for trial in range(20):
        a = rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))
        b = rng.standard_normal(n)
        ex = R.exact_dot(a, b)
        assert ex == _frac_dot(a, b)
        assert B.nearest(ex, F64) == R.fsum_dot(a, b)
        lo, hi = R.bracket(ex, F32)
        want = lo if abs(Fraction(lo) - ex) < abs(Fraction(hi) - ex) else hi  # no tie in random data
        assert B.nearest(ex, F32) == want


def test_nearest_breaks_constructed_ties_to_even():
    for dt, p in ((F64, 53), (F32, 24)):
        t = np.dtype(dt).type
        for x in (t(1.0), t(1.5), t(3.0), np.nextafter(t(1.0), t(2.0)), np.nextafter(t(2.0), t(1.0)), t(2.0 ** -100), t(-1.25)):
            up = np.nextafter(x, t(np.inf))
            lo, hi = float(x), float(up)
            mid = (Fraction(lo) + Fraction(hi)) / 2
            even = lo if B._is_even(lo, dt) else hi
            assert B._is_even(lo, dt) != B._is_even(hi, dt)
            assert B.nearest(mid, dt) == even
            eps = Fraction(1, 1 << 200)
            assert B.nearest(mid + eps, dt) == hi and B.nearest(mid - eps, dt) == lo
            assert B.nearest(Fraction(lo), dt) == lo
    # a tie as a sum of products: 2^53 + 1 = (2^27)(2^26) + 1 * 1 lies half way between 2^53 and 2^53 + 2
    a, b = np.array([2.0 ** 27, 1.0]), np.array([2.0 ** 26, 1.0])
    assert R.exact_dot(a, b) == 2 ** 53 + 1 and B.nearest(R.exact_dot(a, b), F64) == 2.0 ** 53
    a, b = np.array([2.0 ** 27, 1.0, 1.0]), np.array([2.0 ** 26, 1.0, 2.0])
    assert B.nearest(R.exact_dot(a, b), F64) == 2.0 ** 53 + 4   # 2^53 + 3: the even neighbour is above
    assert B.nearest(Fraction(0), F64) == 0.0 and math.copysign(1.0, B.nearest(Fraction(0), F64)) == 1.0


def test_stored_rounds_twice_for_f32():
    """double(T(acc.value())) in an f32 context: a sum just above a float tie becomes the tie when rounded to double, and the
    tie then goes to the even float -- not to the float nearest to the exact sum"""
    mid = (Fraction(1) + Fraction(float(np.nextafter(F32(1), F32(2))))) / 2
    ex = mid + Fraction(1, 1 << 80)
    assert B.nearest(ex, F32) == float(np.nextafter(F32(1), F32(2)))
    assert B.stored(ex, F32) == 1.0
    assert B.stored(ex, F64) == float(mid)
    assert B.check_rounded(1.0, ex, Fraction(0), F32) == "ok"
    # the mutation "rounded once": the float nearest to the exact sum is NOT what the kernels store
    assert B.check_rounded(B.nearest(ex, F32), ex, Fraction(0), F32) == "wrong"
    assert B.check_rounded(B.nearest(ex, F32), ex, B.dd_bound(10, 1), F32) == "wrong"


# ---------------------------------------------------------------- the host double-double sum and its mutations
def _data(n, seed, family="pos"):
    cols, _ = B.family(family, n, 3, seed, F64)
    return cols


def test_two_prod_is_error_free():
    rng = np.random.default_rng(3)
    for x, y in zip(rng.standard_normal(200) * np.exp2(rng.integers(-30, 30, 200)), rng.standard_normal(200)):
        p, e = B.two_prod(float(x), float(y))
        assert Fraction(p) + Fraction(e) == Fraction(float(x)) * Fraction(float(y))


@pytest.mark.parametrize("n,chunks", [(1, 1), (64, 1), (257, 4), (5000, 64)])
@pytest.mark.parametrize("family", ["pos", "indep", "spread"])
def test_a_correct_double_double_sum_passes(n, chunks, family):
    a, b, _ = _data(n, 11, family)
    hi, lo = B.dd_dot(a, b, min(chunks, n))
    ex = R.exact_dot(a, b)
    bound = B.dd_bound(n, R.exact_dot(np.abs(a), np.abs(b)))
    B.check_pair(hi, lo, ex, bound)
    assert B.check_rounded(hi + lo, ex, bound, F64) == "ok"
    assert hi + lo == B.nearest(ex, F64)


MUT_N = 5000


@pytest.fixture(scope="module")
def correct():
    a, b, c = _data(MUT_N, 12)
    rows = np.random.default_rng(13).random(MUT_N) < 0.6
    rows[100] = False
    rows[200] = True
    ex = R.exact_dot(a[rows], b[rows])
    bound = B.dd_bound(int(rows.sum()), R.exact_dot(np.abs(a[rows]), np.abs(b[rows])))
    hi, lo = B.dd_dot(a[rows], b[rows], 64)
    B.check_pair(hi, lo, ex, bound)
    assert B.check_rounded(hi + lo, ex, bound, F64) == "ok"
    assert not B.is_ambiguous(ex, bound, F64)
    return a, b, c, rows, ex, bound


def _rejected(hi, lo, ex, bound, pair_too=True):
    assert B.check_rounded(hi + lo, ex, bound, F64) == "wrong"
    if pair_too:
        with pytest.raises(AssertionError):
            B.check_pair(hi, lo, ex, bound)


def test_mutation_one_ulp_off(correct):
    a, b, c, rows, ex, bound = correct
    good = B.nearest(ex, F64)
    for off in (np.nextafter(good, np.inf), np.nextafter(good, -np.inf)):
        assert B.check_rounded(off, ex, bound, F64) == "wrong"
        assert R.adjacent(off, ex, F64) or True   # (statement_ref's weaker criterion may accept one of them: the point of this file)
    # the bracket value on the other side of the exact sum passes `adjacent` and fails here
    lo_, hi_ = R.bracket(ex, F64)
    other = hi_ if good == lo_ else lo_
    assert R.adjacent(other, ex, F64) and B.check_rounded(other, ex, bound, F64) == "wrong"
    with pytest.raises(AssertionError):
        B.check_pair(other, 0.0, ex, bound)


def test_mutation_row_dropped_counted_twice_or_masked_out_row_included(correct):
    a, b, c, rows, ex, bound = correct
    idx = np.flatnonzero(rows)
    dropped = np.delete(idx, len(idx) - 1)            # the tail row
    _rejected(*B.dd_dot(a[dropped], b[dropped], 64), ex, bound)
    dropped = np.delete(idx, 0)
    _rejected(*B.dd_dot(a[dropped], b[dropped], 64), ex, bound)
    twice = np.append(idx, idx[len(idx) // 2])
    _rejected(*B.dd_dot(a[twice], b[twice], 64), ex, bound)
    assert not rows[100]
    extra = np.append(idx, 100)
    _rejected(*B.dd_dot(a[extra], b[extra], 64), ex, bound)
    # ... even the smallest row of a "spread" input, thirteen decades below the largest, moves the un-rounded pair
    sa, sb, _ = _data(MUT_N, 14, "spread")
    k = int(np.argmin(np.abs(sa * sb)))
    keep = np.arange(MUT_N) != k
    sex = R.exact_dot(sa, sb)
    sbound = B.dd_bound(MUT_N, R.exact_dot(np.abs(sa), np.abs(sb)))
    B.check_pair(*B.dd_dot(sa, sb, 64), sex, sbound)
    if abs(Fraction(float(sa[k])) * Fraction(float(sb[k]))) > sbound:
        with pytest.raises(AssertionError):
            B.check_pair(*B.dd_dot(sa[keep], sb[keep], 64), sex, sbound)


def test_mutation_lo_discarded_at_one_merge(correct):
    a, b, c, rows, ex, bound = correct
    for k in (0, 31, 62):
        hi, lo = B.dd_dot(a[rows], b[rows], 64, drop_lo_at=k)
        with pytest.raises(AssertionError):
            B.check_pair(hi, lo, ex, bound)
    # the rounded value survives such a loss in most entries -- which is why the (hi, lo) pairs are checked on their own --
    # but not in all: over many sums some land on the other side of a rounding boundary
    flipped = 0
    rng = np.random.default_rng(15)
    for trial in range(60):
        x, y = rng.standard_normal(400), rng.standard_normal(400)
        e = R.exact_dot(x, y)
        hi, lo = B.dd_dot(x, y, 8, drop_lo_at=3)
        flipped += B.check_rounded(hi + lo, e, B.dd_bound(400, R.exact_dot(np.abs(x), np.abs(y))), F64) == "wrong"
    assert flipped >= 1


def test_mutation_two_columns_swapped(correct):
    a, b, c, rows, ex, bound = correct
    _rejected(*B.dd_dot(a[rows], c[rows], 64), ex, bound)        # (a, c) where (a, b) was asked for
    cols = [a, b, c]
    good = B.exact_gram(cols, rows)
    swapped = B.exact_gram([a, c, b], rows)
    wrong = [e for e in range(6) if good[e] != swapped[e]]
    assert wrong == [1, 2, 3, 5]   # (1,0) <-> (2,0), (1,1) <-> (2,2); (0,0) and (2,1) are symmetric in the swap
    for e in wrong:
        assert B.check_rounded(B.nearest(swapped[e], F64), good[e], bound, F64) == "wrong"


def test_ambiguity_zone_admits_both_neighbours_and_nothing_else():
    lo, hi = 1.0, float(np.nextafter(1.0, 2.0))
    mid = (Fraction(lo) + Fraction(hi)) / 2
    bound = Fraction(1, 1 << 90)
    ex = mid + bound / 2           # nearest is hi, but an error of `bound` could have crossed the boundary
    assert B.is_ambiguous(ex, bound, F64)
    assert B.check_rounded(hi, ex, bound, F64) == "ok"
    assert B.check_rounded(lo, ex, bound, F64) == "ambiguous-ok"
    assert B.check_rounded(float(np.nextafter(hi, 2.0)), ex, bound, F64) == "wrong"
    assert B.check_rounded(float(np.nextafter(lo, 0.0)), ex, bound, F64) == "wrong"
    assert B.check_rounded(math.nan, ex, bound, F64) == "wrong" and B.check_rounded(math.inf, ex, bound, F64) == "wrong"
    ex = mid + 2 * bound           # outside the zone: only the nearest
    assert not B.is_ambiguous(ex, bound, F64)
    assert B.check_rounded(lo, ex, bound, F64) == "wrong" and B.check_rounded(hi, ex, bound, F64) == "ok"
    # an exactly known sum (B = 0) on the boundary: ties to even, the other neighbour is wrong
    assert B.check_rounded(lo, mid, Fraction(0), F64) == "ok" and B.check_rounded(hi, mid, Fraction(0), F64) == "wrong"
    # the empty sum is +0, not -0
    assert B.check_rounded(0.0, Fraction(0), Fraction(0), F64) == "ok"
    assert B.check_rounded(-0.0, Fraction(0), Fraction(0), F64) == "wrong"
    # judge: more ambiguous entries than the cap is a failure of the input, not a pass
    with pytest.raises(AssertionError, match="uninformative"):
        B.judge([hi], [mid + bound / 2], [bound], F64, 0)
    assert B.judge([lo], [mid + bound / 2], [bound], F64, 1) == 1


def test_sum_bound_is_zero_only_where_the_sum_is_provably_exact():
    rng = np.random.default_rng(16)
    a = rng.standard_normal(300).astype(F32)
    b = rng.standard_normal(300).astype(F32)
    sab = R.exact_dot(np.abs(a), np.abs(b))
    assert B.sum_bound(300, sab, a, b) == 0
    # the compensated double sum of the exact products is then the exact sum, whatever the order
    terms = a.astype(F64) * b.astype(F64)
    for order in (np.arange(300), rng.permutation(300)):
        hi = lo = 0.0
        for t in terms[order].tolist():
            s, err = B.two_sum(hi, t)
            lo += err
            hi = s
        assert Fraction(hi) + Fraction(lo) == R.exact_dot(a, b)
    # doubles against v = -1 (the bound selectors): exact too, and the host double-double sum shows it for any chunking
    w = rng.standard_normal(300)
    v = np.full(300, -1.0)
    assert B._lowbit_exp(v) == 0 and B._lowbit_exp(np.array([0.0, 0.75, -6.0])) == -2
    assert B.sum_bound(300, R.exact_dot(np.abs(w), np.abs(v)), w, v) == 0
    for chunks in (1, 7, 64):
        hi, lo = B.dd_dot(w, v, chunks)
        assert Fraction(hi) + Fraction(lo) == R.exact_dot(w, v)
    # full 53-bit doubles against each other, or data spread over many binades: the general bound
    w2 = rng.standard_normal(300)
    sab = R.exact_dot(np.abs(w), np.abs(w2))
    assert B.sum_bound(300, sab, w, w2) == B.dd_bound(300, sab) > 0
    wide = a.copy()
    wide[0] = F32(2.0 ** -120)
    wide[1] = F32(2.0 ** 100)
    sab = R.exact_dot(np.abs(wide), np.abs(b))
    assert B.sum_bound(300, sab, wide, b) == B.dd_bound(300, sab)
    assert B.sum_bound(5, 0, np.zeros(5, F32), b[:5]) == 0


def test_i8_bound_restates_the_header():
    assert B.i8_bound(1000, 2.0, 3.0) == 1000 * Fraction(6, 1 << 80)
    # the two parts of the derivation stay below the whole: 2^-83 + 2^-80.6 < 2^-80
    dropped = sum((s + 1) * 2 ** 14 * 256 ** s for s in range(10))
    assert Fraction(dropped, 1 << 172) * 4 + Fraction(1, 1 << 83) < Fraction(1, 1 << 80)


# ---------------------------------------------------------------- the prologue statement
@pytest.mark.parametrize("dt", [F64, F32])
def test_gp_linear_restatement_equals_a_plain_loop(dt):
    rng = np.random.default_rng(17)
    n, t = 50, 6
    cols = [rng.standard_normal(n).astype(dt) for _ in range(t)]
    g = rng.standard_normal(n).astype(dt)
    g[3] = dt(-0.0)
    coef = rng.standard_normal(t)
    cF, v = B.gp_linear_ref(cols, coef, g, dt)
    for i in range(n):
        a = dt(0)
        for j in range(t):
            a = dt(a + dt(cols[j][i] * dt(coef[j])))
        want = dt(dt(dt(-1) * a) + g[i])
        assert cF[i] == want and v[i] == -want
    cF0, v0 = B.gp_linear_ref(cols, None, g, dt)
    assert np.array_equal(cF0, g) and np.array_equal(v0, -g)
    assert cF0.dtype == dt and v.dtype == dt


# ---------------------------------------------------------------- the inputs of the GPU file
def test_case_builder_places_every_row_as_intended():
    for cs in (B.ROW_CASES[3], B.MASK_CASES[3], B.MASK_CASES[6], B.WRAP_CASES[0], B.F32_CASES[0]):
        bt = B.build_case(cs)
        dt = np.dtype(cs.dtype).type
        assert all(c.dtype == dt for c in bt.cols) and bt.g.dtype == dt and bt.drt.dtype == dt
        assert len(bt.cols) == 2 * bt.c and bt.c == min(cs.npairs, cs.m)
        # break points of k_cauchy_build in T (x0 = 0) against the threshold 1
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(bt.lb == bt.ub, dt(0), np.where(bt.g < 0, (dt(0) - bt.ub) / bt.g,
                                                         np.where(bt.g > 0, (dt(0) - bt.lb) / bt.g, dt(np.inf))))
        assert np.array_equal(bt.state == B.ST_FREE, t > 1) and np.array_equal(bt.state == B.ST_NEWACT, (t > 0) & (t <= 1))
        assert np.array_equal(bt.free, bt.state == B.ST_FREE) and np.isfinite(bt.drt).all()
        # logical column j = the newest pair in storage slot j
        for j in range(bt.c):
            k = max(k for k in range(cs.npairs) if k % cs.m == j)
            assert bt.cols[j] is bt.pairs[k][1] and bt.cols[bt.c + j] is bt.pairs[k][0]
    one = B.build_case(B.MASK_CASES[3])
    assert np.flatnonzero(one.free).tolist() == [63]
    wrap = B.build_case(B.WRAP_CASES[0])
    assert wrap.cols[0] is wrap.pairs[5][1] and wrap.cols[3] is wrap.pairs[3][1]   # m = 5, 8 pairs: slots 0..2 were overwritten
    pos = B.build_case(B.ROW_CASES[9])
    assert (pos.cols[0][pos.free] * pos.drt[pos.free] >= 0).all()   # v follows base's sign: the v row is as well conditioned


@pytest.mark.parametrize("cs", B.all_cases(), ids=B.case_id)
def test_ambiguity_precondition_of_every_gpu_case(cs):
    """"pos" and "spread": no exact sum within its bound of a rounding boundary; "indep": at most one in twenty.  Needs only
    the exact sums and the bound, so it is decided here; the GPU tests assert the same cap again (bounded_sums_ref.judge)."""
    masks = (0,) if cs is B.I8_FLUSH_CASE else (0, B.ST_FREE)
    for mask in masks:
        gram, wtv = B.case_sums(cs, mask)
        ex, bd = gram.exact + wtv.exact, gram.bound + wtv.bound
        amb = sum(1 for e, b in zip(ex, bd) if B.is_ambiguous(e, b, F64))
        assert amb <= B.cap_for(cs.family, len(ex)), "%d of %d" % (amb, len(ex))
        if cs.family != "indep":
            assert amb == 0
