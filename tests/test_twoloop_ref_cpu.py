"""CPU proof of tests/twoloop_ref.py, the exact reference of the two-loop recursion:
  * it equals a scalar transcription of BFGSMat.h:276-302 (Python floats / np.float32 scalars, Fraction dots);
  * it equals the oracle's apply_Hv (double-double accumulators) bit for bit on every element;
  * each of eight plausible wrong variants of the recursion is told apart from it on the inputs the GPU file uses;
  * no dot of any small GPU case lies within the accumulator's bound of a rounding boundary (a condition of the GPU file,
    asserted here on the reference alone: the seeds in twoloop_ref were chosen so that it holds)."""
from fractions import Fraction

import numpy as np
import pytest

import bounded_sums_ref as B
import oracle_lib as O
import statement_ref as R
import twoloop_ref as T

DT = {O.F64: np.float64, O.F32: np.float32}


# ---------------------------------------------------------------- the scalar transcription
def _fdot(a, b, dt):
    """the exact dot in Fractions, rounded once to double (Fraction -> float is correctly rounded) and then, for f32, to float"""
    ex = sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))
    return dt(float(ex))


def scalar_apply_Hv(pairs, m, v, a, dt):
    """BFGSMat::add_correction + apply_Hv (BFGSMat.h:81-97, 276-302), statement by statement on lists of T scalars"""
    n = len(v)
    m_s, m_y, m_ys = [None] * m, [None] * m, [None] * m
    m_theta, m_ncorr, m_ptr = dt(1), 0, m
    for s, y in pairs:
        loc = m_ptr % m
        m_s[loc], m_y[loc] = [dt(t) for t in s], [dt(t) for t in y]
        m_ys[loc] = _fdot(m_s[loc], m_y[loc], dt)
        m_theta = _fdot(m_y[loc], m_y[loc], dt) / m_ys[loc]
        m_ncorr = min(m_ncorr + 1, m)
        m_ptr = loc + 1
    dots = []
    res = [dt(a) * dt(t) for t in v]
    alpha = [None] * m
    j = m_ptr % m
    for _ in range(m_ncorr):
        j = (j + m - 1) % m
        dots.append(_fdot(m_s[j], res, dt))
        alpha[j] = dots[-1] / m_ys[j]
        res = [dt(r - dt(alpha[j] * yy)) for r, yy in zip(res, m_y[j])]
    res = [dt(r / m_theta) for r in res]
    for _ in range(m_ncorr):
        dots.append(_fdot(m_y[j], res, dt))
        beta = dots[-1] / m_ys[j]
        res = [dt(r + dt(dt(alpha[j] - beta) * ss)) for r, ss in zip(res, m_s[j])]
        j = (j + 1) % m
    dots.append(_fdot([dt(t) for t in v], res, dt))
    assert all(type(r) is dt for r in res) and len(res) == n
    return np.array(res, dt), dots, m_theta


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 7, 50])
def test_reference_equals_the_scalar_transcription(dt, n):
    m = 3
    for npairs in range(0, m + 3):       # c = 0 .. m, then the ring wrapped once and twice
        for a in (-1.0, 1.0, 0.75):
            rng = np.random.default_rng([5, n, npairs])
            pairs = []
            for _ in range(npairs):
                s = rng.standard_normal(n)
                pairs.append((s.astype(dt), (s * (1.0 + rng.random(n)) + 0.05 * rng.standard_normal(n)).astype(dt)))
            v = rng.standard_normal(n).astype(dt)
            want_d, want_dots, want_theta = scalar_apply_Hv(pairs, m, v, a, dt)
            S, Y, ptr = T.ring_fill(pairs, m)
            got = T.two_loop(S, Y, ptr, m, v, a, None, dt)
            assert got.d.dtype == dt and np.array_equal(got.d, want_d), (npairs, a)
            assert [float(d.value) for d in got.dots] == [float(d) for d in want_dots]
            assert float(got.theta) == float(want_theta) and got.dg == float(want_dots[-1])
            assert len(got.dots) == 2 * min(npairs, m) + 1


def test_ring_order_follows_the_pointer():
    assert T.ring_order(3, 3, 0) == [] and T.ring_order(2, 5, 2) == [1, 0]
    assert T.ring_order(5, 5, 5) == [4, 3, 2, 1, 0] and T.ring_order(3, 5, 5) == [2, 1, 0, 4, 3]
    pairs = [(np.full(2, float(k)), np.full(2, float(k))) for k in range(1, 9)]
    S, Y, ptr = T.ring_fill(pairs, 5)
    assert ptr == 3 and [int(S[j][0]) for j in range(5)] == [6, 7, 8, 4, 5]
    assert [int(S[j][0]) for j in T.ring_order(ptr, 5, 5)] == [8, 7, 6, 5, 4]


def test_stored_dot_is_the_correctly_rounded_exact_sum():
    rng = np.random.default_rng(3)
    for dt in (np.float64, np.float32):
        a, b = rng.standard_normal(301).astype(dt), rng.standard_normal(301).astype(dt)
        d = T.rdot(a, b, dt)
        assert type(d.value) is dt and float(d.value) == float(dt(R.fsum_dot(a, b))) and d.exact == R.exact_dot(a, b)
        assert d.bound >= 0 and not d.ambiguous
    # an exact tie of the double rounding is ambiguous under dd_bound (f64) and decided, ties to even, where the sum is exact
    a = np.array([1.0, 2.0 ** -53], np.float64)
    d = T.rdot(a, np.ones(2), np.float64)
    assert d.ambiguous and float(d.value) == 1.0


# ---------------------------------------------------------------- the oracle
ORACLE_SHAPES = [(1000, 6, 0), (1000, 6, 3), (4099, 6, 6), (4099, 5, 13), (65537, 10, 10), (2, 3, 2), (7, 3, 5), (3001, 32, 35),
                 (3001, 33, 33), (2050, 70, 75), (1030, 128, 131), (1030, 129, 133), (515, 200, 60)]  # test_apply_Hv_matches_oracle's


def hv_inputs(dtype, n, m, npairs):
    """the inputs of tests/test_lbfgs_gpu.py::test_apply_Hv_matches_oracle"""
    rng = np.random.default_rng(1234 + n + npairs)
    dt = DT[dtype]
    S = rng.standard_normal((max(npairs, 1), n)).astype(dt)
    Y = (S * (1.0 + rng.random((max(npairs, 1), n))) + 0.05 * rng.standard_normal((max(npairs, 1), n))).astype(dt)
    return S[:npairs], Y[:npairs], rng.standard_normal(n).astype(dt)


@pytest.mark.parametrize("dtype", [O.F64, O.F32])
@pytest.mark.parametrize("n,m,npairs", ORACLE_SHAPES)
def test_oracle_equals_the_exact_reference_on_every_element(oracle, dtype, n, m, npairs):
    S, Y, v = hv_inputs(dtype, n, m, npairs)
    want = oracle.apply_Hv(dtype, m, S.reshape(npairs, n), Y.reshape(npairs, n), v, -1.0)
    Ss, Ys, ptr = T.ring_fill([(S[k], Y[k]) for k in range(npairs)], m)
    got = T.two_loop(Ss, Ys, ptr, m, v, -1.0, None, DT[dtype])
    assert not got.ambiguous
    assert np.array_equal(got.d, want)


@pytest.mark.parametrize("cs", [c for c in T.small_cases() if c.n <= 70000 and c.family != "other"], ids=T.case_id)
def test_oracle_equals_the_exact_reference_on_the_gpu_cases(oracle, cs):
    bt = T.built(cs)
    dtype = O.F64 if cs.dtype == np.float64 else O.F32
    k = len(bt.pairs)
    S = np.stack([p[0] for p in bt.pairs]) if k else np.zeros((0, cs.n), cs.dtype)
    Y = np.stack([p[1] for p in bt.pairs]) if k else np.zeros((0, cs.n), cs.dtype)
    want = oracle.apply_Hv(dtype, cs.m, S, Y, bt.v, bt.a)
    assert np.array_equal(T.reference(cs)[3].d, want)


# ---------------------------------------------------------------- the wrong variants
def _fma(a, b, c):
    """a * b + c with one rounding (f32: exact in double, one further rounding; f64: TwoProd and TwoSum, then the error terms)"""
    if a.dtype == np.float32 or b.dtype == np.float32:
        return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)
    a = np.broadcast_to(np.float64(a), c.shape)
    p = a * b
    ah, al = R._split(a)
    bh, bl = R._split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    return s + (err + e)


def _seq_dot(a, b, dt):
    """the dot accumulated left to right in plain T (products rounded to T too)"""
    return dt(np.cumsum(a * b, dtype=dt)[-1]) if a.size else dt(0)


VARIANTS = ["fma", "alpha_by_reciprocal", "difference_before_division", "theta_by_reciprocal", "theta_of_oldest", "storage_order",
            "sequential_dot", "last_dot_against_v"]


def mutated_two_loop(S, Y, ptr, m, v, a, g, dt, variant):
    """two_loop with one thing wrong; returns (d, [dot values], g.d)"""
    c = 0 if S is None else len(S)
    order = T.ring_order(c if variant == "storage_order" else ptr, m, c)
    dot = (lambda x, y: _seq_dot(x, y, dt)) if variant == "sequential_dot" else (lambda x, y: T.rdot(x, y, dt).value)
    ys = {j: T.rdot(S[j], Y[j], dt).value for j in order}
    th = {j: T.rdot(Y[j], Y[j], dt).value / ys[j] for j in order}
    dots, alpha = [], {}
    q = dt(a) * v
    for j in order:
        dots.append(dot(S[j], q))
        alpha[j] = dots[-1] * (dt(1) / ys[j]) if variant == "alpha_by_reciprocal" else dots[-1] / ys[j]
        q = _fma(-alpha[j], Y[j], q) if variant == "fma" else q - alpha[j] * Y[j]
    if c:
        theta = th[order[-1]] if variant == "theta_of_oldest" else th[order[0]]
        q = q * (dt(1) / theta) if variant == "theta_by_reciprocal" else q / theta
    for j in reversed(order):
        dots.append(dot(Y[j], q))
        if variant == "difference_before_division":
            coef = (dots[order.index(j)] - dots[-1]) / ys[j]
        else:
            coef = alpha[j] - dots[-1] / ys[j]
        q = _fma(coef, S[j], q) if variant == "fma" else q + coef * S[j]
    dots.append(dot(v if (g is None or variant == "last_dot_against_v") else g, q))
    return q, [float(d) for d in dots], float(dots[-1])


def test_the_unmutated_restatement_is_the_reference():
    for cs in (T.HISTORY[3], T.HISTORY[4], T.FAMILIES[1], T.OTHER_V[0], T.HISTORY[-1]):
        bt = T.built(cs)
        S, Y, ptr, ref = T.reference(cs)
        d, dots, dg = mutated_two_loop(S, Y, ptr, cs.m, bt.v, bt.a, bt.g, cs.dtype, None)
        assert np.array_equal(d, ref.d) and dots == [float(x.value) for x in ref.dots] and dg == ref.dg


def _applicable(variant, cs):
    c = min(cs.npairs, cs.m)
    if variant == "last_dot_against_v":
        return cs.family == "other"
    if variant == "sequential_dot":
        return cs.n >= 64          # below that a left-to-right sum in T is often the correctly rounded one
    if variant == "storage_order":
        return cs.npairs > cs.m and cs.npairs % cs.m != 0 and cs.n >= 4
    if variant == "theta_of_oldest":
        return c >= 2 and cs.n >= 4
    return c >= 1 and cs.n >= 64   # the element-wise and coefficient variants: one rounding among a handful may coincide


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_variant_is_told_apart_on_the_gpu_inputs(variant):
    """On every small GPU case the variant applies to, what the GPU file compares -- d, the dots, the last dot -- differs from
    the reference's: a kernel with this mistake fails there."""
    caught = {np.float64: 0, np.float32: 0}
    for cs in T.small_cases():
        if not _applicable(variant, cs) or cs.n > 70000:
            continue
        bt = T.built(cs)
        S, Y, ptr, ref = T.reference(cs)
        d, dots, dg = mutated_two_loop(S, Y, ptr, cs.m, bt.v, bt.a, bt.g, cs.dtype, variant)
        same = np.array_equal(d, ref.d) and dots == [float(x.value) for x in ref.dots]
        # a variant that changes one scalar per pair leaves that scalar's rounding unchanged about two times in three, and a
        # left-to-right sum in T can be the correctly rounded one: a case with a handful of such scalars may agree by chance
        # (seen here with five pairs); the cases with more than a hundred pairs must not, and must not for a sum per pair
        c = min(cs.npairs, cs.m)
        by_chance = (variant in ("alpha_by_reciprocal", "difference_before_division") and c < 100) or (
            variant == "sequential_dot" and c == 0)
        assert by_chance or not same, "%s is not told apart on %s" % (variant, T.case_id(cs))
        if not same and variant != "last_dot_against_v" and cs.npairs > 0:
            assert not np.array_equal(d, ref.d), "%s leaves d itself unchanged on %s" % (variant, T.case_id(cs))
        caught[cs.dtype] += 0 if same else 1
    assert min(caught.values()) >= 2, "%s: told apart on %r cases only" % (variant, caught)


# ---------------------------------------------------------------- the conditions of the GPU file
@pytest.mark.parametrize("cs", T.small_cases(), ids=T.case_id)
def test_no_dot_of_a_small_gpu_case_is_ambiguous(cs):
    S, Y, ptr, ref = T.reference(cs)
    c = min(cs.npairs, cs.m)
    assert len(ref.dots) == 2 * c + 1 and np.all(np.isfinite(ref.d))
    for k, d in enumerate(ref.dots):
        assert not d.ambiguous, "dot %d of %s lies within %.3g ulp of a rounding boundary" % (
            k, T.case_id(cs), float(d.bound / R.ulp(d.exact, np.float64)))
    for j in ref.order:
        _, _, sy, yy = T.pair_scalars(S[j], Y[j], cs.dtype)
        assert not sy.ambiguous and not yy.ambiguous and sy.value > 0


def test_orth_family_has_a_tiny_first_dot_that_is_still_well_conditioned():
    for cs in T.FAMILIES:
        if cs.family != "orth":
            continue
        bt = T.built(cs)
        S, Y, ptr, ref = T.reference(cs)
        s0, q0 = S[ref.order[0]], cs.dtype(bt.a) * bt.v
        terms = R.dot_terms(s0, q0)
        assert R.well_conditioned(terms, ref.dots[0].exact)
        sabs = float(np.sum(np.abs(s0.astype(np.float64) * q0.astype(np.float64))))
        assert abs(float(ref.dots[0].exact)) < 2.0 ** -12 * sabs


def test_mag_family_spans_sixty_binades():
    for cs in T.FAMILIES:
        if cs.family == "mag":
            bt = T.built(cs)
            e = [np.log2(np.abs(p[0].astype(np.float64)).max()) for p in bt.pairs]
            assert max(e) - min(e) > 55 and np.all(np.isfinite(T.reference(cs)[3].d))


@pytest.mark.parametrize("cs", T.POST_CASES, ids=T.post_case_id)
def test_no_sum_of_a_small_post_case_is_ambiguous(cs):
    S, Y, ptr, post = T.post_reference(cs)
    assert post.accepted == cs.accept
    assert not any(d.ambiguous for d in post.sums) and not post.two_loop.ambiguous
    assert post.ncorr == min(cs.npairs + (1 if cs.accept else 0), cs.m)
    if cs.accept:   # the recursion on the resulting history is the plain one on the same columns
        again = T.two_loop(post.S, post.Y, post.ptr, cs.m, T.post_built(cs).g, -1.0, None, cs.dtype)
        assert np.array_equal(again.d, post.two_loop.d) and again.dg == post.two_loop.dg


def test_quadratic_iterations_have_no_ambiguous_sum():
    for dt, n in T.QUAD_CASES:
        for it in T.quad_reference(dt, n).iters:
            assert not any(d.ambiguous for d in it.post.sums) and not it.post.two_loop.ambiguous
            assert it.dg < 0 and it.post.two_loop.dg < 0
