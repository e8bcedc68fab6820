"""Plain numpy / Python references of the driver statements (lbfgs_kernels.cuh, lbfgsb_kernels.cuh), for the statement-level
tests (tests/test_statement_ref_cpu.py proves them, tests/test_driver_statements_gpu.py uses them).  No oracle library, no GPU.

The contract they restate:
  * element-wise arithmetic is IEEE in the context's scalar type T without contraction, one rounding per source operation:
    numpy in the same dtype, one numpy operation per operation of the kernel text, reproduces every vector bit for bit;
  * sums go through compensated accumulators (reduce.cuh: DD for f64, D1 for f32) and are rounded to T once (twice for f32:
    to double, then to float): the result is one of the two T values that bracket the exact sum of the T-rounded terms;
  * maxima and minima are exact.
"""
import math
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------- exact sums


def _exact_sum_f64(v):
    """exact sum of finite doubles as a Fraction: mantissas as integers, grouped by exponent.  The 53-bit mantissa is cut
    into a signed upper and a non-negative lower half of at most 27 bits, so a group's sums stay below 2^53 for up to 2^26
    elements and np.bincount (which adds in double) adds them exactly."""
    v = np.ascontiguousarray(v, np.float64).ravel()
    assert np.all(np.isfinite(v)), "finite terms only"
    total = 0  # in units of 2^-1200
    step = 1 << 26
    for lo_i in range(0, v.size, step):
        w = v[lo_i:lo_i + step]
        m, e = np.frexp(w)  # w = m 2^e, 0.5 <= |m| < 1
        mant = np.ldexp(m, 53).astype(np.int64)  # exact: |mant| < 2^53
        hi = mant >> 27
        lo = mant & ((1 << 27) - 1)
        idx = (e - e.min()).astype(np.int64)
        shi = np.bincount(idx, weights=hi.astype(np.float64))
        slo = np.bincount(idx, weights=lo.astype(np.float64))
        base = int(e.min()) - 53 + 1200
        assert base >= 0
        for k in range(shi.size):
            if shi[k] != 0.0 or slo[k] != 0.0:
                total += ((int(shi[k]) << 27) + int(slo[k])) << (base + k)
    return Fraction(total, 1 << 1200)


def exact_sum(terms):
    """the exact real sum of the terms (float32 or float64 array, finite) as a Fraction"""
    t = np.asarray(terms)
    assert t.dtype in (np.float32, np.float64)
    if t.size == 0:
        return Fraction(0)
    return _exact_sum_f64(t.astype(np.float64))


def _split(a):
    """Veltkamp: a = hi + lo with at most 26 significant bits each (no overflow for |a| < 2^996)"""
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def dot_terms(a, b):
    """doubles whose exact sum is the exact dot product: float32 products are exact in double; a float64 product is the sum of
    the four exact partial products of the Dekker / Veltkamp halves"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64) and a.shape == b.shape
    if a.dtype == np.float32:
        return a.astype(np.float64) * b.astype(np.float64)
    ah, al = _split(a)
    bh, bl = _split(b)
    return np.concatenate([ah * bh, ah * bl, al * bh, al * bl])


def exact_dot(a, b):
    """the exact real value of sum a_i b_i as a Fraction"""
    if np.asarray(a).size == 0:
        return Fraction(0)
    return _exact_sum_f64(dot_terms(a, b))


def fsum_dot(a, b):
    """the correctly rounded double of the same dot product through math.fsum (an independent route to the same number)"""
    return math.fsum(dot_terms(a, b).tolist())


# ---------------------------------------------------------------- the criterion for a sum
_PREC = {np.dtype(np.float32): (24, -149), np.dtype(np.float64): (53, -1074)}


def _floor_log2(q):
    """floor(log2(q)) of a positive Fraction, exactly"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    return e


def ulp(exact, dtype):
    """spacing of dtype's values in the binade of |exact| (the smallest subnormal at and around zero), as a Fraction"""
    p, emin = _PREC[np.dtype(dtype)]
    exact = Fraction(exact)
    if exact == 0:
        return Fraction(2) ** emin
    return Fraction(2) ** max(_floor_log2(abs(exact)) - (p - 1), emin)


def bracket(exact, dtype):
    """(lo, hi): the largest dtype value <= exact and the smallest >= exact (equal when exact is a dtype value)"""
    t = np.dtype(dtype).type
    exact = Fraction(exact)
    c = t(float(exact))  # near exact (rounded twice for float): walk from there
    assert np.isfinite(c), "the exact value is outside dtype's range"
    while Fraction(float(c)) > exact:
        c = np.nextafter(c, t(-np.inf))
    while Fraction(float(np.nextafter(c, t(np.inf)))) <= exact:
        c = np.nextafter(c, t(np.inf))
    lo = c
    hi = lo if Fraction(float(lo)) == exact else np.nextafter(lo, t(np.inf))
    return float(lo), float(hi)


def adjacent(got, exact, dtype):
    """True when `got` (a value of dtype, handed over widened to a Python float) is one of the two dtype values that bracket
    the exact real value -- which implies |got - exact| < ulp_T(exact); an exactly representable value admits itself alone.
    Derived, not measured: the compensated accumulator errs by about n 2^-104 sum|t_i| (below 2^-60 relative under
    well_conditioned), then come one rounding to double and, for f32, a second one to float -- which is why the criterion
    is "adjacent" and not "correctly rounded"."""
    got = float(got)
    if not math.isfinite(got):
        return False
    ok = got in bracket(exact, dtype)
    assert not ok or abs(Fraction(got) - Fraction(exact)) < ulp(exact, dtype)
    return ok


def well_conditioned(terms, exact):
    """sum|t_i| <= 2^20 |sum t_i|: the precondition of `adjacent` (sum|t_i| taken in double, rounded up generously)"""
    sabs = float(np.sum(np.abs(np.asarray(terms, np.float64)))) * (1.0 + 1e-9)
    return Fraction(sabs) <= (1 << 20) * abs(Fraction(exact))


def check_sum(got, terms, dtype, scale=1):
    """(ok, message) for a kernel's sum over `terms` (doubles whose exact sum is the sum meant), times the exact factor `scale`"""
    ex = _exact_sum_f64(terms) if np.asarray(terms).size else Fraction(0)
    assert well_conditioned(terms, ex), "test input is ill-conditioned: sum|t| > 2^20 |sum t|, choose another seed"
    ex = ex * Fraction(scale)
    ok = adjacent(got, ex, dtype)
    return ok, "got %r, exact %.20g (+- ulp %.3g), off by %.3g ulp" % (got, float(ex), float(ulp(ex, dtype)),
                                                                      float((Fraction(float(got)) - ex) / ulp(ex, dtype))
                                                                      if math.isfinite(float(got)) else float("nan"))


def check_dot(got, a, b, dtype):
    return check_sum(got, dot_terms(a, b), dtype)


# ---------------------------------------------------------------- objectives: (gradient, the T-rounded terms of f, factor)
# the kernels add the terms to the accumulator as T values and apply `factor` (OBJ::finish) to the T-rounded sum; the two
# factors that occur, 1 and 0.5, are exact


def quad_ref(x, a, b):
    """ObjQuad (lbfgs_kernels.cuh): r = a x - b; g = a r; term r r; f = 0.5 sum"""
    dt = x.dtype.type
    r = a * x - b
    return a * r, r * r, Fraction(1, 2)


def rosen_ref(x):
    """ObjRosen: pairs (x[2k], x[2k+1])"""
    dt = x.dtype.type
    x0, x1 = x[0::2], x[1::2]
    t1 = dt(1) - x0
    t2 = dt(10) * (x1 - x0 * x0)
    g = np.empty_like(x)
    g1 = dt(20) * t2
    g[1::2] = g1
    g[0::2] = dt(-2) * (x0 * g1 + t1)
    return g, t1 * t1 + t2 * t2, Fraction(1)


# A term over two coordinates whose data depends on the index: the term that starts at i reads p0[i], p0[i+1], p1[i], p1[i+1].
# Only + - *: every operation is one IEEE rounding on the device and in numpy.
CHAIN2 = """const T t = p0[i] * x[0] - p1[i + 1] * x[1];
const T q = p0[i + 1] * x[0];
const T u = x[1] - q * x[0];
g[0] = (T(2) * (t * p0[i]) - T(4) * (u * q)) + p1[i];
g[1] = T(2) * u - T(2) * (t * p1[i + 1]);
return (t * t + u * u) + p1[i] * x[0];"""


def chain2_ref(x, p0, p1):
    dt = x.dtype.type
    x0, x1 = x[0::2], x[1::2]
    p0a, p0b, p1a, p1b = p0[0::2], p0[1::2], p1[0::2], p1[1::2]
    t = p0a * x0 - p1b * x1
    q = p0b * x0
    u = x1 - q * x0
    g = np.empty_like(x)
    g[0::2] = (dt(2) * (t * p0a) - dt(4) * (u * q)) + p1a
    g[1::2] = dt(2) * u - dt(2) * (t * p1b)
    return g, (t * t + u * u) + p1a * x0, Fraction(1)


# One coordinate per term, all four data slots and all eight scalars, each in a role of its own (and one division, which is
# correctly rounded on the device as in numpy).  p3 + c[5] must stay away from zero.
ALLSLOTS = """const T a = (p0[i] * x[0] - c[0]) * c[1];
const T b = (p1[i] + c[2]) * x[0] - c[3];
const T w = p3[i] + c[5];
const T e = (p2[i] * c[4] + x[0] / w) - c[6];
g[0] = (T(2) * a) * (p0[i] * c[1]) + (T(2) * b) * (p1[i] + c[2]) + ((T(2) * c[7]) * e) / w;
return (a * a + b * b) + c[7] * (e * e);"""
# eight distinct values, none representable in float (nor, 0.1-like, in double): the library converts them with T(c)
ALLSLOTS_SCALARS = (0.1, 1.3, 0.7, 0.2, 1.7, 2.3, 0.3, 0.9)


def allslots_ref(x, p0, p1, p2, p3, scalars=ALLSLOTS_SCALARS):
    dt = x.dtype.type
    c = [dt(v) for v in scalars]  # launch_args.hpp term_args: T(c)
    a = (p0 * x - c[0]) * c[1]
    b = (p1 + c[2]) * x - c[3]
    w = p3 + c[5]
    e = (p2 * c[4] + x / w) - c[6]
    g = (dt(2) * a) * (p0 * c[1]) + (dt(2) * b) * (p1 + c[2]) + ((dt(2) * c[7]) * e) / w
    return g, (a * a + b * b) + c[7] * (e * e), Fraction(1)


# ---------------------------------------------------------------- element-wise statements


def axpy_ref(xp, d, step):
    """x = xp + step d with the step converted to T first (k_trial, k_axpy_point, k_b_dg_maxstep_trial)"""
    dt = xp.dtype.type
    return xp + dt(step) * d


def clamp_ref(x, lb, ub):
    """k_force_bounds: v = (v < lb) ? lb : v; v = (ub < v) ? ub : v"""
    v = np.where(x < lb, lb, x)
    return np.where(ub < v, ub, v)


def projg_terms_ref(x, g, lb, ub):
    """projg_term (lbfgsb_kernels.cuh): |clamp(x - g, lb, ub) - x| per coordinate, in T"""
    v = clamp_ref(x - g, lb, ub) - x
    return np.where(v < 0, -v, v)


def projg_norm_ref(x, g, lb, ub):
    """the kernels' maximum starts from 0.0 and is exact"""
    t = projg_terms_ref(x, g, lb, ub)
    return float(t.max()) if t.size else 0.0


def step_max_ref(x, d, lb, ub):
    """k_b_dg_maxstep / feas: the minimum over d_i != 0 of double((bound_i - x_i) / d_i) + 0.0 (the quotient in T; the + 0.0
    turns -0 into +0 before fmin sees it), started from +inf, converted to T"""
    dt = x.dtype.type
    pos, neg = d > 0, d < 0
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        q = np.concatenate([(ub[pos] - x[pos]) / d[pos], (lb[neg] - x[neg]) / d[neg]])
    q = q.astype(np.float64) + 0.0
    return float(dt(q.min())) if q.size else math.inf


def sy_ref(x, xp, g, gp):
    """s = x - xp, y = g - gp (k_post, k_b_post)"""
    return x - xp, g - gp


def dir_from_xcp_ref(xcp, x):
    """k_b_dir_from_xcp: d = xcp - x"""
    return xcp - x


def normalized_candidates(d):
    """lbfgsx_b_dir_from_xcp(normalize = 1): z = T(d.d) from the compensated sum, then -- when z > 0 -- d_i / T(sqrt(z)) with
    the square root taken in T on the host (k_b_scale_div).  z is adjacent to the exact d.d, so there are at most two admissible
    results: the list of them, the one from the correctly rounded z first."""
    dt = d.dtype.type
    ex = exact_dot(d, d)
    if ex == 0:
        return [d.copy()]
    near = dt(float(ex)) if d.dtype == np.float64 else dt(np.float64(float(ex)))
    cands = [near]
    for other in (np.nextafter(near, dt(0)), np.nextafter(near, dt(np.inf))):
        if adjacent(float(other), ex, d.dtype):
            cands.append(other)
    out = []
    for z in cands:
        out.append(d / np.sqrt(z) if z > 0 else d.copy())
    return out


# ---------------------------------------------------------------- scalar restatements (plain loops), for the CPU proofs


def step_max_scalar(x, d, lb, ub):
    dt = x.dtype.type
    smin = math.inf
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for i in range(x.size):
            if d[i] > dt(0):
                smin = min(smin, float(dt((ub[i] - x[i]) / d[i])) + 0.0)
            elif d[i] < dt(0):
                smin = min(smin, float(dt((lb[i] - x[i]) / d[i])) + 0.0)
    return float(dt(smin))


def projg_scalar(x, g, lb, ub):
    dt = x.dtype.type
    pg = 0.0
    for i in range(x.size):
        v = dt(x[i] - g[i])
        v = lb[i] if v < lb[i] else v
        v = ub[i] if ub[i] < v else v
        v = dt(v - x[i])
        v = -v if v < dt(0) else v
        pg = max(pg, float(v))
    return pg


# ---------------------------------------------------------------- the shapes the statement tests run at
def edge_sizes(dtype, big=True):
    """W = elements per 16-byte pack, tile = 256 x 4 packs (k_trial, k_post); the grid of the streaming kernels is capped at
    1024 blocks of 256 packs, so above 1024 * 256 * W elements every block walks several strides"""
    W = 2 if np.dtype(dtype) == np.float64 else 4
    tile = 256 * 4
    ns = [1, 2, 3, W - 1, W, W + 1, 2 * W + 1, 256 * W - 1, 256 * W, 256 * W + 1, tile * W - 1, tile * W, tile * W + 1,
          tile * W + W + 1, 3 * tile * W + 5]
    if big:
        ns += [1024 * 256 * W + 2 * tile * W + W + 1, 3_000_001]
    out = []
    for n in ns:
        if n >= 1 and n not in out:
            out.append(n)
    return out


def nearest_even(n):
    return n if n % 2 == 0 else n + 1


# ---------------------------------------------------------------- inputs shared by the CPU proofs and the GPU tests
def bound_cases(rng, n, dt):
    """name -> (x, d, lb, ub): the bound edges every bounded statement is run on; x inside [lb, ub] except where said"""
    inf = dt(np.inf)
    x = rng.standard_normal(n).astype(dt)
    d = rng.standard_normal(n).astype(dt)
    lo = (x - (0.5 + rng.random(n))).astype(dt)
    hi = (x + (0.5 + rng.random(n))).astype(dt)
    cases = {}
    cases["all_infinite"] = (x, d, np.full(n, -inf, dt), np.full(n, inf, dt))
    cases["d_zero"] = (x, np.zeros(n, dt), lo, hi)
    lb, ub, xx = lo.copy(), hi.copy(), x.copy()
    pin = rng.random(n) < 0.3
    pin[0] = True
    ub[pin] = lb[pin]
    xx[pin] = lb[pin]
    cases["lb_eq_ub"] = (xx, d, lb, ub)
    # x exactly on a bound, d pointing outward: the quotient is -0 or +0, step_max must be +0
    xx, dd = x.copy(), d.copy()
    k = n // 2
    xx[k] = hi[k]
    dd[k] = abs(dd[k]) + dt(0.25)
    cases["on_bound_outward_upper"] = (xx, dd, lo, hi)
    xx, dd = x.copy(), d.copy()
    xx[k] = lo[k]
    dd[k] = -abs(dd[k]) - dt(0.25)
    cases["on_bound_outward_lower"] = (xx, dd, lo, hi)
    # the limiting coordinate placed: vector body (0), last whole pack, scalar tail (last element)
    W = 2 if dt == np.float64 else 4
    for name, k in (("limit_first", 0), ("limit_last_pack", max(0, (n // W) * W - 1)), ("limit_tail", n - 1)):
        lb, ub = lo.copy(), hi.copy()
        ub[k] = x[k] + dt(2.0 ** -12) * (dt(1) + dt(rng.random()))
        lb[k] = x[k] - dt(2.0 ** -12) * (dt(1) + dt(rng.random()))
        dd = d.copy()
        dd[k] = dt(1.5) if rng.random() < 0.5 else dt(-1.5)
        cases[name] = (x, dd, lb, ub)
    lb, ub = lo.copy(), hi.copy()
    lb[rng.random(n) < 0.5] = -inf
    ub[rng.random(n) < 0.5] = inf
    cases["mixed_one_sided"] = (x, d, lb, ub)
    return cases


def term_data(rng, n, dt):
    """four data arrays whose every element differs, p3 kept positive (ALLSLOTS divides by p3 + c[5])"""
    return [(0.5 + rng.random(n)).astype(dt), (rng.random(n) - 0.5).astype(dt), (1.0 + rng.random(n)).astype(dt),
            (0.25 + rng.random(n)).astype(dt)]
