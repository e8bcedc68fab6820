"""Grid field objectives (lbfgspp_amd.GridFieldObjective; csrc/grid_field_kernels.cuh): the bodies the tests compile and their
plain numpy restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x is node-major: x.reshape(rows, cols, D)[r, c, d] is unknown d of node (r, c); `mask` has bit 0 for the columns and bit 1 for
the rows, as in periodic_ref.  A restatement returns (tg, v) on the FULL grid: tg[k*D + d][origin] the partial derivative of
the cell with that origin by unknown d of its corner k -- corner 2*dr + dc is node origin + (dr, dc) modulo the extents -- and
v[origin] its value, computed for every origin whether the cell exists or not; exists(shape, mask) says which do.  field_grad
puts the gradient together by the rule of include/lbfgsx.h ("grid field objectives"): per node and unknown the cells
(r-1, c-1), (r-1, c), (r, c-1), (r, c), those that exist, started from the first.  The bodies use + - * only."""
import itertools
import math

import numpy as np

import periodic_ref as PR

FASYM_SCALARS = (0.375, -0.625)
# every corner and component weighted by p0 at its flat coordinate j[k]*D + d, with a multiplier of its own, so that a wrong
# seam index, a swapped slot or a swapped component changes bits
FASYM = """T w[4 * D];
T s = T(0);
#pragma unroll
for (int k = 0; k < 4; k++)
{
#pragma unroll
    for (int d = 0; d < D; d++)
    {
        w[k * D + d] = p0[j[k] * D + d] * T(1 + 2 * k + 7 * d);
        s = s + w[k * D + d] * x[k * D + d];
    }
}
const T q = s + (T(row) * c[0] + T(col) * c[1]);
#pragma unroll
for (int m = 0; m < 4 * D; m++)
    g[m] = w[m] * q;
return T(0.5) * (q * q);"""
# Ginzburg-Landau: a, b, e, h the edge differences x1-x0, x2-x0, x3-x2, x3-x1 of component d; the cell's value is
# 1/4 sum_d ((a^2+b^2)+(e^2+h^2)) + (c0/4) (sum_d x0_d^2 - 1)^2
GL = """T ss = T(0);
#pragma unroll
for (int d = 0; d < D; d++)
    ss = ss + x[d] * x[d];
const T u = ss - T(1);
const T k = c[0] * T(0.25);
T v = T(0);
#pragma unroll
for (int d = 0; d < D; d++)
{
    const T a = x[D + d] - x[d];
    const T b = x[2 * D + d] - x[d];
    const T e = x[3 * D + d] - x[2 * D + d];
    const T h = x[3 * D + d] - x[D + d];
    g[d] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[d]);
    g[D + d] = T(0.5) * (a - h);
    g[2 * D + d] = T(0.5) * (b - e);
    g[3 * D + d] = T(0.5) * (e + h);
    v = v + ((a * a + b * b) + (e * e + h * h));
}
return T(0.25) * v + k * (u * u);"""


def exists(shape, mask):
    return PR.exists(shape, mask)


def corners(a, shape, D):
    """corners[k][d]: the full-grid array of unknown d of corner k of the cell with that origin, from a flat per-coordinate array"""
    A = a.reshape(tuple(shape) + (D,))
    return [[np.roll(A[:, :, d], (-dr, -dc), axis=(0, 1)) for d in range(D)] for dr, dc in PR.offsets(2)]


def fasym_terms(x, shape, D, p0, scalars=FASYM_SCALARS):
    dt = x.dtype.type
    xc, pc = corners(x, shape, D), corners(p0, shape, D)
    row, col = PR._coords(shape, x.dtype)
    w = [None] * (4 * D)
    s = np.zeros(shape, x.dtype)
    for k in range(4):
        for d in range(D):
            w[k * D + d] = pc[k][d] * dt(1 + 2 * k + 7 * d)
            s = s + w[k * D + d] * xc[k][d]
    q = s + (row * dt(scalars[0]) + col * dt(scalars[1]))
    return [wm * q for wm in w], dt(0.5) * (q * q)


def gl_terms(x, shape, D, c0):
    dt = x.dtype.type
    xc = corners(x, shape, D)
    ss = np.zeros(shape, x.dtype)
    for d in range(D):
        ss = ss + xc[0][d] * xc[0][d]
    u = ss - dt(1)
    k = dt(c0) * dt(0.25)
    tg = [None] * (4 * D)
    v = np.zeros(shape, x.dtype)
    for d in range(D):
        a = xc[1][d] - xc[0][d]
        b = xc[2][d] - xc[0][d]
        e = xc[3][d] - xc[2][d]
        h = xc[3][d] - xc[1][d]
        tg[d] = dt(-0.5) * (a + b) + (dt(4) * k) * (u * xc[0][d])
        tg[D + d] = dt(0.5) * (a - h)
        tg[2 * D + d] = dt(0.5) * (b - e)
        tg[3 * D + d] = dt(0.5) * (e + h)
        v = v + ((a * a + b * b) + (e * e + h * h))
    return tg, dt(0.25) * v + k * (u * u)


def field_grad(tg, shape, D, mask):
    """flat node-major gradient: per unknown d the periodic grid rule on the four arrays tg[k*D + d]"""
    assert len(tg) == 4 * D
    g = np.empty(tuple(shape) + (D,), tg[0].dtype)
    for d in range(D):
        g[:, :, d] = PR.periodic_grad([tg[k * D + d] for k in range(4)], shape, mask).reshape(shape)
    return g.reshape(-1)


def field_grad_scalar(tg, shape, D, mask):
    """the same rule as a plain loop over nodes and unknowns, written out from the header's four lines (the proof of
    field_grad); also counts how often each cell's slots were used"""
    dt = tg[0].dtype.type
    rows, cols = shape
    pc, pr = bool(mask & 1), bool(mask & 2)
    g = np.zeros((rows, cols, D), tg[0].dtype)
    used = np.zeros((rows, cols, 4 * D), np.int64)
    for r, c, d in itertools.product(range(rows), range(cols), range(D)):
        acc = None
        for k, (dr, dc) in ((3, (1, 1)), (2, (1, 0)), (1, (0, 1)), (0, (0, 0))):
            orr, oc = r - dr, c - dc
            if (orr < 0 and not pr) or (oc < 0 and not pc):
                continue
            orr, oc = orr % rows, oc % cols
            if (orr == rows - 1 and not pr) or (oc == cols - 1 and not pc):
                continue
            t = tg[k * D + d][orr, oc]
            used[orr, oc, k * D + d] += 1
            acc = t if acc is None else dt(acc + t)
        g[r, c, d] = acc
    return g.reshape(-1), used


def value_exact(v, shape, mask):
    return math.fsum(float(t) for t in v[exists(shape, mask)])


def values(v, shape, mask):
    """the existing cells' values as a flat array (for statement_ref's exact sums)"""
    return v[exists(shape, mask)].reshape(-1)
