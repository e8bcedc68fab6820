"""Periodic grid and volume objectives (lbfgspp_amd.PeriodicGridObjective, PeriodicVolumeObjective;
csrc/periodic_grid_kernels.cuh, csrc/periodic_volume_kernels.cuh): the bodies the tests compile and their plain numpy
restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x is a row-major array of `shape` = (rows, cols) or (slabs, rows, cols); `mask` has bit 0 for the last axis (columns), bit 1
for the rows, bit 2 for the slabs.  A restatement returns (tg, v) on the FULL shape: tg[j][origin] the j-th partial derivative
of the cell with that origin -- slot 2*dr + dc (4*ds + 2*dr + dc) is node origin + (ds, dr, dc) modulo the extents -- and
v[origin] its value, computed for every origin whether the cell exists or not; exists(shape, mask) says which do.
periodic_grad puts the gradient together by the rule of include/lbfgsx.h: per node the cells origin = node - (ds, dr, dc),
all offsets 1 first, in ascending binary order of (1-ds, 1-dr, 1-dc), those that exist, started from the first.  The bodies
use + - * only."""
import itertools
import math

import numpy as np

import grid_ref
import volume_ref

# the statement tests' bodies: grid_ref.ASYM4 and volume_ref.ASYM8 with p0 read at every corner through j, so that a wrong
# seam index changes bits
PASYM4 = """const T w0 = p0[j[0]], w1 = p0[j[1]], w2 = p0[j[2]], w3 = p0[j[3]];
const T s = ((w0 * x[0] + T(2) * (w1 * x[1])) + T(3) * (w2 * x[2])) + T(5) * (w3 * x[3]);
const T q = s + (T(row) * c[0] + T(col) * c[1]);
g[0] = w0 * q;
g[1] = T(2) * (w1 * q);
g[2] = T(3) * (w2 * q);
g[3] = T(5) * (w3 * q);
return T(0.5) * (q * q);"""
PASYM8 = """const T w0 = p0[j[0]], w1 = p0[j[1]], w2 = p0[j[2]], w3 = p0[j[3]];
const T w4 = p0[j[4]], w5 = p0[j[5]], w6 = p0[j[6]], w7 = p0[j[7]];
const T s0 = ((w0 * x[0] + T(2) * (w1 * x[1])) + T(3) * (w2 * x[2])) + T(5) * (w3 * x[3]);
const T s1 = ((T(7) * (w4 * x[4]) + T(11) * (w5 * x[5])) + T(13) * (w6 * x[6])) + T(17) * (w7 * x[7]);
const T q = (s0 + s1) + ((T(slab) * c[0] + T(row) * c[1]) + T(col) * c[2]);
g[0] = w0 * q;
g[1] = T(2) * (w1 * q);
g[2] = T(3) * (w2 * q);
g[3] = T(5) * (w3 * q);
g[4] = T(7) * (w4 * q);
g[5] = T(11) * (w5 * q);
g[6] = T(13) * (w6 * q);
g[7] = T(17) * (w7 * q);
return T(0.5) * (q * q);"""
# the Allen-Cahn energies are the open forms' texts: they read no data and no position
ALLENCAHN = grid_ref.ALLENCAHN
ALLENCAHN3 = volume_ref.ALLENCAHN3


def offsets(nd):
    """the corner offsets in slot order: (dr, dc) or (ds, dr, dc)"""
    return list(itertools.product((0, 1), repeat=nd))


def corners(a, shape):
    """the 2^nd full-shape arrays of a flat per-node array: slot k of the cell with origin [idx] is corners[k][idx]"""
    A = a.reshape(shape)
    return [np.roll(A, tuple(-o for o in off), axis=tuple(range(len(shape)))) for off in offsets(len(shape))]


def axis_periodic(shape, mask, ax):
    return bool(mask >> (len(shape) - 1 - ax) & 1)


def exists(shape, mask):
    """which origins have a cell: per axis, not the last layer or the axis is periodic"""
    e = np.ones(shape, bool)
    for ax, ext in enumerate(shape):
        if not axis_periodic(shape, mask, ax):
            idx = np.arange(ext).reshape([-1 if k == ax else 1 for k in range(len(shape))])
            e = e & (idx < ext - 1)
    return e


def _coords(shape, dtype):
    return [np.arange(ext).astype(dtype).reshape([-1 if k == ax else 1 for k in range(len(shape))]) for ax, ext in enumerate(shape)]


def pasym4_terms(x, shape, p0, scalars=grid_ref.ASYM_SCALARS):
    dt = x.dtype.type
    x0, x1, x2, x3 = corners(x, shape)
    w0, w1, w2, w3 = corners(p0, shape)
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    row, col = _coords(shape, x.dtype)
    s = ((w0 * x0 + dt(2) * (w1 * x1)) + dt(3) * (w2 * x2)) + dt(5) * (w3 * x3)
    q = s + (row * c0 + col * c1)
    return [w0 * q, dt(2) * (w1 * q), dt(3) * (w2 * q), dt(5) * (w3 * q)], dt(0.5) * (q * q)


def pasym8_terms(x, shape, p0, scalars=volume_ref.ASYM_SCALARS):
    dt = x.dtype.type
    x0, x1, x2, x3, x4, x5, x6, x7 = corners(x, shape)
    w0, w1, w2, w3, w4, w5, w6, w7 = corners(p0, shape)
    c0, c1, c2 = dt(scalars[0]), dt(scalars[1]), dt(scalars[2])
    slab, row, col = _coords(shape, x.dtype)
    s0 = ((w0 * x0 + dt(2) * (w1 * x1)) + dt(3) * (w2 * x2)) + dt(5) * (w3 * x3)
    s1 = ((dt(7) * (w4 * x4) + dt(11) * (w5 * x5)) + dt(13) * (w6 * x6)) + dt(17) * (w7 * x7)
    q = (s0 + s1) + ((slab * c0 + row * c1) + col * c2)
    tg = [w0 * q, dt(2) * (w1 * q), dt(3) * (w2 * q), dt(5) * (w3 * q), dt(7) * (w4 * q), dt(11) * (w5 * q), dt(13) * (w6 * q),
          dt(17) * (w7 * q)]
    return tg, dt(0.5) * (q * q)


def allencahn_terms(x, shape, c0):
    dt = x.dtype.type
    x0, x1, x2, x3 = corners(x, shape)
    a = x1 - x0
    b = x2 - x0
    e = x3 - x2
    h = x3 - x1
    u = x0 * x0 - dt(1)
    k = dt(c0) * dt(0.25)
    tg = [dt(-0.5) * (a + b) + (dt(4) * k) * (u * x0), dt(0.5) * (a - h), dt(0.5) * (b - e), dt(0.5) * (e + h)]
    return tg, dt(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u)


def allencahn3_terms(x, shape, c0):
    dt = x.dtype.type
    x0, x1, x2, x3, x4, x5, x6, x7 = corners(x, shape)
    a0, a1, a2, a3 = x1 - x0, x3 - x2, x5 - x4, x7 - x6
    b0, b1, b2, b3 = x2 - x0, x3 - x1, x6 - x4, x7 - x5
    e0, e1, e2, e3 = x4 - x0, x5 - x1, x6 - x2, x7 - x3
    u = x0 * x0 - dt(1)
    k = dt(c0) * dt(0.25)
    tg = [dt(-0.25) * ((a0 + b0) + e0) + (dt(4) * k) * (u * x0),
          dt(0.25) * ((a0 - b1) - e1),
          dt(0.25) * ((b0 - a1) - e2),
          dt(0.25) * ((a1 + b1) - e3),
          dt(0.25) * ((e0 - a2) - b2),
          dt(0.25) * ((a2 + e1) - b3),
          dt(0.25) * ((b2 + e2) - a3),
          dt(0.25) * ((a3 + b3) + e3)]
    sa = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)
    sb = (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3)
    se = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3)
    return tg, dt(0.125) * ((sa + sb) + se) + k * (u * u)


def order(nd):
    """(slot, offset) of a node's cells in the order of the adds: the cell at node - offset holds the node in `slot`"""
    return [(sum(o << (nd - 1 - k) for k, o in enumerate(off)), off) for off in reversed(offsets(nd))]


def periodic_grad(tg, shape, mask):
    """flat gradient: per node the contributions of the cells it is a corner of, in the fixed order, no leading 0 +"""
    dt = tg[0].dtype
    nd = len(shape)
    axes = tuple(range(nd))
    assert min(shape) >= 2 and all(a.shape == tuple(shape) and a.dtype == dt for a in tg)
    ex = exists(shape, mask)
    g = np.zeros(shape, dt)
    has = np.zeros(shape, bool)
    for slot, off in order(nd):
        c = np.roll(tg[slot], off, axis=axes)
        # on an open axis node 0 has no cell before it: the roll brings the last layer there, which holds no cell
        valid = np.roll(ex, off, axis=axes)
        g =np.where(valid, np.where(has, g + c, c), g)
        has |= valid
    assert has.all() and g.dtype == dt
    return g.reshape(-1)


def periodic_grad_scalar(tg, shape, mask):
    """the same rule as a plain loop over the nodes (the proof of periodic_grad); also counts how often each cell's slots
    were used, returned as the second value: every existing cell must be used once per slot, no other cell at all"""
    dt = tg[0].dtype.type
    nd = len(shape)
    g = np.zeros(shape, tg[0].dtype)
    used = np.zeros(tuple(shape) + (2 ** nd,), np.int64)
    for node in itertools.product(*(range(e) for e in shape)):
        acc = None
        for slot, off in order(nd):
            origin, ok = [], True
            for ax in range(nd):
                o = node[ax] - off[ax]
                per = axis_periodic(shape, mask, ax)
                if o < 0:
                    ok = ok and per
                    o += shape[ax]
                if o == shape[ax] - 1 and not per:
                    ok = False
                origin.append(o)
            if ok:
                v = tg[slot][tuple(origin)]
                used[tuple(origin) + (slot,)] += 1
                acc = v if acc is None else dt(acc + v)
        g[node] = acc
    return g.reshape(-1), used


def value_exact(v, shape, mask):
    """the exact sum of the existing cells' values, rounded once to a double"""
    return math.fsum(float(t) for t in v[exists(shape, mask)])


def values(v, shape, mask):
    """the existing cells' values as a flat array (for statement_ref's exact sums)"""
    return v[exists(shape, mask)].reshape(-1)
