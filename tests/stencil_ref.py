"""Grid stencil objectives (lbfgspp_amd.StencilObjective; csrc/grid_stencil_kernels.cuh): the bodies the tests compile and
their plain numpy restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x is a row-major array of `shape` = (rows, cols), rows >= 3 and cols >= 3; `mask` has bit 0 for the columns and bit 1 for the
rows.  A restatement returns (tg, v) on the FULL shape: tg[k][origin] the k-th partial derivative of the patch with that origin
-- slot 3*dr + dc is node origin + (dr, dc) modulo the extents -- and v[origin] its value, computed for every origin whether
the patch exists or not; exists(shape, mask) says which do.  stencil_grad puts the gradient together by the rule of
include/lbfgsx.h: per node the patches origin = node - (dr, dc), dr = 2, 1, 0 (outer) and dc = 2, 1, 0 (inner), those that
exist, started from the first.  The bodies use + - * only."""
import itertools
import math

import numpy as np

MULT = (1, 2, 3, 5, 7, 11, 13, 17, 19)  # SASYM9's multiplier of slot k
SASYM_SCALARS = (0.0625, -0.03125)      # c[0], c[1]: the weights of row and col

# every slot weighted by p0 read through j with a multiplier of its own, and the position of slot 0: a wrong seam index, a
# swapped slot or a wrong (row, col) changes bits
SASYM9 = """const T w0 = p0[j[0]], w1 = p0[j[1]], w2 = p0[j[2]], w3 = p0[j[3]], w4 = p0[j[4]];
const T w5 = p0[j[5]], w6 = p0[j[6]], w7 = p0[j[7]], w8 = p0[j[8]];
const T s0 = (w0 * x[0] + T(2) * (w1 * x[1])) + T(3) * (w2 * x[2]);
const T s1 = (T(5) * (w3 * x[3]) + T(7) * (w4 * x[4])) + T(11) * (w5 * x[5]);
const T s2 = (T(13) * (w6 * x[6]) + T(17) * (w7 * x[7])) + T(19) * (w8 * x[8]);
const T q = ((s0 + s1) + s2) + (T(row) * c[0] + T(col) * c[1]);
g[0] = w0 * q;
g[1] = T(2) * (w1 * q);
g[2] = T(3) * (w2 * q);
g[3] = T(5) * (w3 * q);
g[4] = T(7) * (w4 * q);
g[5] = T(11) * (w5 * q);
g[6] = T(13) * (w6 * q);
g[7] = T(17) * (w7 * q);
g[8] = T(19) * (w8 * q);
return T(0.5) * (q * q);"""

# a Swift-Hohenberg / plate energy: half the squared five-point Laplacian at the patch's centre plus a double well of weight
# c[0] on the centre.  It reads no data and no position
PLATE = """const T l = (((x[1] + x[3]) + x[5]) + x[7]) - T(4) * x[4];
const T u = x[4] * x[4] - T(1);
const T kw = c[0] * T(0.25);
g[0] = T(0);
g[2] = T(0);
g[6] = T(0);
g[8] = T(0);
g[1] = l;
g[3] = l;
g[5] = l;
g[7] = l;
g[4] = T(-4) * l + (T(4) * kw) * (u * x[4]);
return T(0.5) * (l * l) + kw * (u * u);"""

# the text of a 2x2 cell (a PeriodicGridObjective's: x[4], g[4], j[4]) as a stencil body on the slots {0, 1, 3, 4}
SUB2X2 = """const T y[4] = {x[0], x[1], x[3], x[4]};
const int64_t jj[4] = {j[0], j[1], j[3], j[4]};
T h[4];
const T v = [&](const T (&x)[4], T (&g)[4], const int64_t (&j)[4]) -> T {
%s
}(y, h, jj);
g[0] = h[0];
g[1] = h[1];
g[3] = h[2];
g[4] = h[3];
g[2] = T(0);
g[5] = T(0);
g[6] = T(0);
g[7] = T(0);
g[8] = T(0);
return v;"""

# a chain term of K = 3 that reads neither data nor its index, and the same text on the first row of a patch
CHAIN3 = """const T a = x[1] - x[0] * x[0];
const T b = x[2] - x[1];
g[0] = T(-2) * (a * x[0]);
g[1] = a - b;
g[2] = b;
return T(0.5) * (a * a + b * b);"""
ROW3 = """const T y[3] = {x[0], x[1], x[2]};
T h[3];
const T v = [&](const T (&x)[3], T (&g)[3]) -> T {
%s
}(y, h);
g[0] = h[0];
g[1] = h[1];
g[2] = h[2];
g[3] = T(0);
g[4] = T(0);
g[5] = T(0);
g[6] = T(0);
g[7] = T(0);
g[8] = T(0);
return v;""" % CHAIN3


def offsets():
    """the node offsets (dr, dc) in slot order"""
    return list(itertools.product((0, 1, 2), repeat=2))


def nodes(a, shape):
    """the nine full-shape arrays of a flat per-node array: slot k of the patch with origin [idx] is nodes[k][idx]"""
    A = a.reshape(shape)
    return [np.roll(A, (-dr, -dc), axis=(0, 1)) for dr, dc in offsets()]


def axis_periodic(mask, ax):
    return bool(mask >> (1 - ax) & 1)


def exists(shape, mask):
    """which origins have a patch: per axis, not the last two layers or the axis is periodic"""
    e = np.ones(shape, bool)
    for ax, ext in enumerate(shape):
        if not axis_periodic(mask, ax):
            idx = np.arange(ext).reshape([-1 if k == ax else 1 for k in range(2)])
            e = e & (idx < ext - 2)
    return e


def _coords(shape, dtype):
    return [np.arange(ext).astype(dtype).reshape([-1 if k == ax else 1 for k in range(2)]) for ax, ext in enumerate(shape)]


def sasym9_terms(x, shape, p0, scalars=SASYM_SCALARS):
    dt = x.dtype.type
    x0, x1, x2, x3, x4, x5, x6, x7, x8 = nodes(x, shape)
    w = nodes(p0, shape)
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    row, col = _coords(shape, x.dtype)
    s0 = (w[0] * x0 + dt(2) * (w[1] * x1)) + dt(3) * (w[2] * x2)
    s1 = (dt(5) * (w[3] * x3) + dt(7) * (w[4] * x4)) + dt(11) * (w[5] * x5)
    s2 = (dt(13) * (w[6] * x6) + dt(17) * (w[7] * x7)) + dt(19) * (w[8] * x8)
    q = ((s0 + s1) + s2) + (row * c0 + col * c1)
    tg = [w[0] * q] + [dt(MULT[k]) * (w[k] * q) for k in range(1, 9)]
    return tg, dt(0.5) * (q * q)


def plate_terms(x, shape, c0):
    dt = x.dtype.type
    _, x1, _, x3, x4, x5, _, x7, _ = nodes(x, shape)
    l = (((x1 + x3) + x5) + x7) - dt(4) * x4
    u = x4 * x4 - dt(1)
    kw = dt(c0) * dt(0.25)
    z = np.zeros(shape, x.dtype)
    tg = [z, l, z, l, dt(-4) * l + (dt(4) * kw) * (u * x4), l, z, l, z]
    return tg, dt(0.5) * (l * l) + kw * (u * u)


def order():
    """(slot, offset) of a node's patches in the order of the adds: the patch at node - offset holds the node in `slot`"""
    return [(3 * dr + dc, (dr, dc)) for dr in (2, 1, 0) for dc in (2, 1, 0)]


def stencil_grad(tg, shape, mask):
    """flat gradient: per node the contributions of the patches it is a node of, in the fixed order, no leading 0 +"""
    dt = tg[0].dtype
    assert min(shape) >= 3 and all(a.shape == tuple(shape) and a.dtype == dt for a in tg)
    ex = exists(shape, mask)
    g = np.zeros(shape, dt)
    has = np.zeros(shape, bool)
    for slot, off in order():
        c = np.roll(tg[slot], off, axis=(0, 1))
        # on an open axis the nodes 0 and 1 have no patch two before them, node 0 none one before: the roll brings the last
        # two layers there, which hold no patch
        valid = np.roll(ex, off, axis=(0, 1))
        g = np.where(valid, np.where(has, g + c, c), g)
        has |= valid
    assert has.all() and g.dtype == dt
    return g.reshape(-1)


def stencil_grad_scalar(tg, shape, mask):
    """the rule of include/lbfgsx.h written out as a plain loop over the nodes (the proof of stencil_grad); also counts how
    often each patch's slots were used, returned as the second value: every existing patch must be used once per slot, no other
    patch at all"""
    dt = tg[0].dtype.type
    rows, cols = shape
    pr, pc = bool(mask & 2), bool(mask & 1)
    g = np.zeros(shape, tg[0].dtype)
    used = np.zeros(tuple(shape) + (9,), np.int64)
    for r in range(rows):
        for c in range(cols):
            acc = None
            for dr in (2, 1, 0):
                for dc in (2, 1, 0):
                    orow, ocol = r - dr, c - dc
                    if (orow < 0 and not pr) or (ocol < 0 and not pc):
                        continue  # on an open axis a negative origin means the patch does not exist
                    orow, ocol = orow % rows, ocol % cols
                    if not ((ocol < cols - 2 or pc) and (orow < rows - 2 or pr)):
                        continue
                    v = tg[3 * dr + dc][orow, ocol]
                    used[orow, ocol, 3 * dr + dc] += 1
                    acc = v if acc is None else dt(acc + v)
            g[r, c] = acc
    return g.reshape(-1), used


def value_exact(v, shape, mask):
    """the exact sum of the existing patches' values, rounded once to a double"""
    return math.fsum(float(t) for t in v[exists(shape, mask)])


def values(v, shape, mask):
    """the existing patches' values as a flat array (for statement_ref's exact sums)"""
    return v[exists(shape, mask)].reshape(-1)
