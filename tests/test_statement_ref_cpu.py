"""CPU suite: the references of tests/statement_ref.py are proved here before the GPU statement tests
(tests/test_driver_statements_gpu.py) rely on them: the exact sums against rational arithmetic, the objective references
against the oracle bit for bit, the scalar statements against plain loops; and the two new term bodies compile for gfx950
without a device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import statement_ref as R

DTYPES = [np.float64, np.float32]


def _frac_sum(v):
    s = Fraction(0)
    for t in v:
        s += Fraction(float(t))
    return s


def _frac_dot(a, b):
    s = Fraction(0)
    for p, q in zip(a, b):
        s += Fraction(float(p)) * Fraction(float(q))
    return s


def _ill_conditioned(rng, n, dt):
    """magnitudes over ~60 binades (20 for float) with heavy cancellation"""
    span = 60 if dt == np.float64 else 20
    v = (rng.standard_normal(n) * np.exp2(rng.integers(-span // 2, span // 2, n))).astype(dt)
    return np.concatenate([v, -v[::-1][: n // 2], rng.standard_normal(3).astype(dt)])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 7, 100, 1500])
def test_exact_sum_and_dot_equal_rational_arithmetic(dt, n):
    rng = np.random.default_rng(100 + n)
    for v in (rng.standard_normal(n).astype(dt), _ill_conditioned(rng, n, dt), np.zeros(n, dt),
              np.full(n, np.finfo(dt).tiny, dt) * dt(0.5), np.full(n, np.finfo(dt).max, dt) * dt(2.0 ** -30)):
        assert R.exact_sum(v) == _frac_sum(v)
        # math.fsum is the correctly rounded double of the same number
        assert float(R.exact_sum(v)) == math.fsum(v.astype(np.float64).tolist())
    for a, b in ((rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)),
                 (_ill_conditioned(rng, n, dt), _ill_conditioned(rng, n, dt)[::-1].copy())):
        assert R.exact_dot(a, b) == _frac_dot(a, b)
        assert float(R.exact_dot(a, b)) == R.fsum_dot(a, b)
    assert R.exact_sum(np.zeros(0, dt)) == 0 and R.exact_dot(np.zeros(0, dt), np.zeros(0, dt)) == 0


def test_exact_sum_where_numpy_is_wrong():
    v = np.array([1e16, 1.0, -1e16, 1.0])
    assert R.exact_sum(v) == 2 and float(np.sum(v)) != 2.0
    # a long one: pairwise summation loses the small terms too
    w = np.concatenate([np.full(1000, 1e16), np.ones(1000), np.full(1000, -1e16), np.ones(1000)])
    assert R.exact_sum(w) == 2000 and float(np.sum(w)) != 2000.0
    a = np.array([2.0 ** 27 + 1.0, 1.0, -(2.0 ** 27 + 1.0)])
    b = np.array([2.0 ** 27 + 1.0, 1.0, 2.0 ** 27 - 1.0])
    # (2^27 + 1)^2 + 1 - (2^54 - 1) = 2^28 + 3
    assert R.exact_dot(a, b) == 2 ** 28 + 3 and float(np.dot(a, b)) != float(2 ** 28 + 3)


def test_exact_sum_in_blocks_of_many_elements():
    """more elements than one exactly added block holds is not testable in CPU test time; the grouping by exponent is: many
    elements per exponent, sums of mantissa halves far above 2^27"""
    rng = np.random.default_rng(5)
    v = rng.standard_normal(300_000)
    assert float(R.exact_sum(v)) == math.fsum(v.tolist())
    f = rng.standard_normal(300_000).astype(np.float32)
    assert float(R.exact_sum(f)) == math.fsum(f.astype(np.float64).tolist())
    assert float(R.exact_dot(v, v[::-1].copy())) == R.fsum_dot(v, v[::-1].copy())


@pytest.mark.parametrize("dt", DTYPES)
def test_adjacent_is_the_two_bracketing_values(dt):
    one = dt(1.0)
    up, down = np.nextafter(one, dt(2)), np.nextafter(one, dt(0))
    eps = Fraction(float(up)) - 1
    assert R.ulp(1, dt) == eps and R.ulp(Fraction(float(down)), dt) == eps / 2
    ex = 1 + eps / 3  # between 1 and up
    assert R.adjacent(float(one), ex, dt) and R.adjacent(float(up), ex, dt)
    assert not R.adjacent(float(down), ex, dt) and not R.adjacent(float(np.nextafter(up, dt(2))), ex, dt)
    # an exactly representable sum admits that value alone
    assert R.adjacent(1.0, 1, dt) and not R.adjacent(float(up), 1, dt) and not R.adjacent(float(down), 1, dt)
    # just below a power of two: the upper neighbour is the power itself
    ex = 1 - eps / 8
    assert R.adjacent(1.0, ex, dt) and R.adjacent(float(down), ex, dt) and not R.adjacent(float(up), ex, dt)
    assert R.adjacent(0.0, 0, dt) and not R.adjacent(float(np.finfo(dt).smallest_subnormal), 0, dt)
    assert R.adjacent(-float(up), -(1 + eps / 3), dt) and not R.adjacent(float(up), -(1 + eps / 3), dt)
    assert not R.adjacent(math.inf, 1, dt) and not R.adjacent(math.nan, 1, dt)
    if dt == np.float32:
        assert not R.adjacent(1.0 + 2.0 ** -30, 1 + eps / 3, dt)  # not a float at all
    t = np.array([1.0, -1.0, 2.0 ** -30], dt)
    assert not R.well_conditioned(t, R.exact_sum(t)) and R.well_conditioned(np.abs(t), R.exact_sum(np.abs(t)))


def _x_for(rng, n, dt):
    return rng.standard_normal(n).astype(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_objective_references_are_bit_identical_to_the_oracle(oracle, dt):
    dtype = O.F64 if dt == np.float64 else O.F32
    sizes = R.edge_sizes(dt, big=False) + [100_003]
    for n in sizes:
        rng = np.random.default_rng(31 + n)
        x = _x_for(rng, n, dt)
        a, b = O.quad_problem(n, dtype=dtype)
        fx_o, g_o = oracle.eval(dtype, O.OBJ_QUAD, x, a, b)
        g, terms, scale = R.quad_ref(x, a, b)
        assert g.dtype == dt and terms.dtype == dt
        assert np.array_equal(g, g_o), "quadratic gradient, n = %d" % n
        ok, msg = R.check_sum(fx_o, terms.astype(np.float64), dt, scale)
        assert ok, "quadratic f, n = %d: %s" % (n, msg)
        if n == 1:  # a single term: the oracle's sum is exact
            assert fx_o == float(dt(0.5) * terms[0])
        ne = R.nearest_even(n)
        xe = _x_for(rng, ne, dt)
        fx_o, g_o = oracle.eval(dtype, O.OBJ_ROSEN, xe)
        g, terms, scale = R.rosen_ref(xe)
        assert g.dtype == dt and terms.dtype == dt and terms.size == ne // 2
        assert np.array_equal(g, g_o), "Rosenbrock gradient, n = %d" % ne
        ok, msg = R.check_sum(fx_o, terms.astype(np.float64), dt, scale)
        assert ok, "Rosenbrock f, n = %d: %s" % (ne, msg)
        if ne == 2:
            assert fx_o == float(terms[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9, 1025])
def test_step_max_and_projected_gradient_equal_scalar_loops(dt, n):
    rng = np.random.default_rng(77 + n)
    for name, (x, d, lb, ub) in R.bound_cases(rng, n, dt).items():
        g = rng.standard_normal(n).astype(dt)
        sm = R.step_max_ref(x, d, lb, ub)
        assert sm == R.step_max_scalar(x, d, lb, ub), name
        if name in ("all_infinite", "d_zero"):
            assert sm == math.inf
        if name.startswith("on_bound_outward"):
            assert sm == 0.0 and math.copysign(1.0, sm) == 1.0, "the quotient -0 must come out as +0"
        if name.startswith("limit_"):
            assert 0 < sm < 2.0 ** -11
        assert R.projg_norm_ref(x, g, lb, ub) == R.projg_scalar(x, g, lb, ub), name
        xo = (x + 3 * rng.standard_normal(n)).astype(dt)  # outside the bounds too
        c = R.clamp_ref(xo, lb, ub)
        assert c.dtype == dt and np.all(c >= lb) and np.all(c <= ub)
        assert np.array_equal(c, np.minimum(np.maximum(xo, lb), ub))
    # without the + 0.0 the on-bound quotient is -0: the reference would not tell the two apart by value, so check the sign
    x = np.array([1.0], dt)
    assert math.copysign(1.0, R.step_max_ref(x, np.array([-2.0], dt), x.copy(), x + 1)) == 1.0


@pytest.mark.parametrize("dt", DTYPES)
def test_new_bodies_tell_indices_slots_and_scalars_apart(dt):
    """what the GPU tests rely on to catch a wrong index, a swapped lane, a permuted slot or scalar: each changes bits of the
    reference's expectation"""
    n = 64
    rng = np.random.default_rng(9)
    x = rng.standard_normal(n).astype(dt)
    p = R.term_data(rng, n, dt)
    g, t, _ = R.chain2_ref(x, p[0], p[1])
    # the index of the pack's first term used for every term of the pack (`vi * W + k` -> `vi * W`)
    W = 2 if dt == np.float64 else 4
    if W > 2:
        first = (np.arange(n) // W) * W + (np.arange(n) % 2)
        g2, t2, _ = R.chain2_ref(x, p[0][first], p[1][first])
        assert not np.array_equal(g, g2) and not np.array_equal(t, t2)
    for shift in (1, 2, -2):
        g2, t2, _ = R.chain2_ref(x, np.roll(p[0], shift), np.roll(p[1], shift))
        assert np.all(g2 != g) and np.all(t2 != t)
    xs = x.reshape(-1, 2)[:, ::-1].reshape(-1).copy()  # lanes of a pair swapped
    assert np.all(R.chain2_ref(xs, p[0], p[1])[0] != g)
    g, t, _ = R.allslots_ref(x, *p)
    for i in range(4):
        for j in range(i + 1, 4):
            q = list(p)
            q[i], q[j] = q[j], q[i]
            g2, t2, _ = R.allslots_ref(x, *q)
            assert np.all(g2 != g) and np.all(t2 != t), (i, j)
    assert len(set(R.ALLSLOTS_SCALARS)) == 8
    for i in range(8):
        assert float(np.float32(R.ALLSLOTS_SCALARS[i])) != R.ALLSLOTS_SCALARS[i]
        for j in range(i + 1, 8):
            c = list(R.ALLSLOTS_SCALARS)
            c[i], c[j] = c[j], c[i]
            g2, t2, _ = R.allslots_ref(x, *p, scalars=c)
            assert np.mean(g2 != g) > 0.9, (i, j)
    if dt == np.float32:  # the scalars rounded to T first, not the arithmetic done in double
        gd, _, _ = R.allslots_ref(x.astype(np.float64), *[q.astype(np.float64) for q in p])
        assert not np.array_equal(gd.astype(np.float32), g)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,K", [("CHAIN2", 2), ("ALLSLOTS", 1)])
def test_new_bodies_compile_without_scratch(dt, name, K):
    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    h = C.c_void_p()
    log = C.create_string_buffer(8192)
    rc = core.lbfgsx_objective_compile(C.byref(h), L.F64 if dt == np.float64 else L.F32, K, getattr(R, name).encode(), log, len(log))
    assert rc == 0 and h.value, log.value.decode()
    info = (C.c_longlong * 8)()
    assert core.lbfgsx_objective_info(h, C.byref(info)) == 0
    print(name, np.dtype(dt).name, list(info))
    assert 0 < info[0] <= 512
    assert info[1] == 0 and list(info[4:8]) == [0, 0, 0, 0], "scratch bytes of k_eval, k_trial, k_b_eval, k_b_dg_maxstep_trial"
    assert core.lbfgsx_objective_K(h) == K
    core.lbfgsx_objective_destroy(h)
