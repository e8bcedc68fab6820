"""Chain objectives (lbfgspp_amd.ChainObjective, csrc/chain_kernels.cuh): the bodies the tests compile and their plain numpy
restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

A restatement returns (tg, v): tg[j][t] the j-th partial derivative of the term that starts at t and v[t] its value, for
t = 0 .. n-K.  chain_grad puts the gradient together by the rule of include/lbfgsx.h: grad[j] is the sum of tg[j-t][t] over
t = max(0, j-K+1) .. min(j, n-K) in ascending t, started from the first contribution."""
import numpy as np

# sum 100 (x[i+1] - x[i]^2)^2 + (1 - x[i])^2
CHAINED_ROSEN = """const T u = x[1] - x[0] * x[0];
const T v = T(1) - x[0];
g[1] = T(200) * u;
g[0] = T(-400) * (u * x[0]) - T(2) * v;
return T(100) * (u * u) + v * v;"""

# sum p0[i] (x[i] - p1[i])^2 + c0 (x[i] - 2 x[i+1] + x[i+2])^2: a weighted fit with a bending-energy regulariser
SECOND_DIFF = """const T r = x[0] - p1[i];
const T s = (x[0] - T(2) * x[1]) + x[2];
const T w = T(2) * (c[0] * s);
g[0] = T(2) * (p0[i] * r) + w;
g[1] = T(-2) * w;
g[2] = w;
return p0[i] * (r * r) + c[0] * (s * s);"""

# the statement tests' bodies: weights that depend on the term's index, the two sides of a term treated differently
# K = 2: p0[i] (x1 - x0^2)^2 + (c0 - x0)^2
ASYM2 = """const T u = x[1] - x[0] * x[0];
const T v = c[0] - x[0];
const T pu = p0[i] * u;
g[1] = T(2) * pu;
g[0] = T(-4) * (pu * x[0]) - T(2) * v;
return pu * u + v * v;"""
# K = 3: p0[i] (x0 - 2 x1 + x2)^2 + c1 x1^4
ASYM3 = """const T s = (x[0] - T(2) * x[1]) + x[2];
const T ps = p0[i] * s;
const T q = x[1] * x[1];
g[0] = T(2) * ps;
g[1] = T(-4) * ps + (T(4) * c[1]) * (q * x[1]);
g[2] = T(2) * ps;
return ps * s + c[1] * (q * q);"""
ASYM_SCALARS = (1.1, 0.3)  # c0, c1: neither is a float or a double

# The extended Rosenbrock function as a chain: the pair term of the built-in ObjRosen (lbfgs_kernels.cuh) with every output
# multiplied by p0[i], which is 1 on even i and 0 on odd i.  Multiplying by 1 and adding +-0 are exact.
ROSEN_MASKED = """const T t1 = T(1) - x[0];
const T t2 = T(10) * (x[1] - x[0] * x[0]);
const T g1 = T(20) * t2;
g[1] = p0[i] * g1;
g[0] = p0[i] * (T(-2) * (x[0] * g1 + t1));
return p0[i] * (t1 * t1 + t2 * t2);"""


def _windows(x, K):
    m = x.size - K + 1
    return [x[j:j + m] for j in range(K)]


def chained_rosen_terms(x):
    dt = x.dtype.type
    x0, x1 = _windows(x, 2)
    u = x1 - x0 * x0
    v = dt(1) - x0
    return [dt(-400) * (u * x0) - dt(2) * v, dt(200) * u], dt(100) * (u * u) + v * v


def second_diff_terms(x, p0, p1, c0):
    dt = x.dtype.type
    m = x.size - 2
    x0, x1, x2 = _windows(x, 3)
    c0 = dt(c0)
    r = x0 - p1[:m]
    s = (x0 - dt(2) * x1) + x2
    w = dt(2) * (c0 * s)
    return [dt(2) * (p0[:m] * r) + w, dt(-2) * w, w], p0[:m] * (r * r) + c0 * (s * s)


def asym2_terms(x, p0, scalars=ASYM_SCALARS):
    dt = x.dtype.type
    m = x.size - 1
    x0, x1 = _windows(x, 2)
    c0 = dt(scalars[0])
    u = x1 - x0 * x0
    v = c0 - x0
    pu = p0[:m] * u
    return [dt(-4) * (pu * x0) - dt(2) * v, dt(2) * pu], pu * u + v * v


def asym3_terms(x, p0, scalars=ASYM_SCALARS):
    dt = x.dtype.type
    m = x.size - 2
    x0, x1, x2 = _windows(x, 3)
    c1 = dt(scalars[1])
    s = (x0 - dt(2) * x1) + x2
    ps = p0[:m] * s
    q = x1 * x1
    return [dt(2) * ps, dt(-4) * ps + (dt(4) * c1) * (q * x1), dt(2) * ps], ps * s + c1 * (q * q)


def chain_grad(tg, n):
    """grad[j] = tg[K-1][j-K+1] (+ ...) + tg[0][j], the terms that exist, ascending t, no leading 0 +"""
    K = len(tg)
    m = n - K + 1
    assert m >= 1 and all(a.size == m for a in tg)
    g = np.zeros(n, tg[0].dtype)
    has = np.zeros(n, bool)
    for o in range(K - 1, -1, -1):  # the term that starts o coordinates before j
        c = np.zeros(n, tg[0].dtype)
        c[o:o + m] = tg[o]
        valid = np.zeros(n, bool)
        valid[o:o + m] = True
        g = np.where(valid, np.where(has, g + c, c), g)
        has |= valid
    assert has.all()
    return g


def chain_grad_scalar(tg, n):
    """the same rule as a plain loop over the coordinates (the proof of chain_grad)"""
    K = len(tg)
    g = np.zeros(n, tg[0].dtype)
    for j in range(n):
        acc = None
        for t in range(max(0, j - K + 1), min(j, n - K) + 1):
            v = tg[j - t][t]
            acc = v if acc is None else tg[0].dtype.type(acc + v)
        g[j] = acc
    return g
