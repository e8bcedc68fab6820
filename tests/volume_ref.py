"""Volume objectives (lbfgspp_amd.VolumeObjective, csrc/volume_kernels.cuh): the bodies the tests compile and their plain
numpy restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x is a slab-major slabs x rows x cols array.  A restatement returns (tg, v): tg[j][s, r, c] the j-th partial derivative of
cell (s, r, c) -- slot 4*ds + 2*dr + dc is node (s+ds, r+dr, c+dc) -- and v[s, r, c] its value, for 0 <= s < slabs-1,
0 <= r < rows-1, 0 <= c < cols-1.  volume_grad puts the gradient together by the rule of include/lbfgsx.h: grad[s, r, c] =
tg[7][s-1, r-1, c-1] + tg[6][s-1, r-1, c] + tg[5][s-1, r, c-1] + tg[4][s-1, r, c] + tg[3][s, r-1, c-1] + tg[2][s, r-1, c] +
tg[1][s, r, c-1] + tg[0][s, r, c], the cells that exist, in this order, started from the first.  The bodies use + - * only."""
import numpy as np

WEIGHTS = (1, 2, 3, 5, 7, 11, 13, 17)

# the statement tests' body: another weight on each slot and each partial, p0 read at all eight corners, slab, row and col in
# the value
#   q = sum_j WEIGHTS[j] w_j x_j + (slab c0 + row c1 + col c2),  value q^2 / 2
ASYM8 = """const int64_t rc = rows * cols;
const T w0 = p0[i], w1 = p0[i + 1], w2 = p0[i + cols], w3 = p0[i + cols + 1];
const T w4 = p0[i + rc], w5 = p0[i + rc + 1], w6 = p0[i + rc + cols], w7 = p0[i + rc + cols + 1];
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
ASYM_SCALARS = (0.3, -0.7, 0.45)  # c0, c1, c2: none is a float or a double

# Allen-Cahn: the squared differences along the cell's twelve edges, each with a quarter of its weight 1/2 (an inner edge
# belongs to four cells), plus the double-well potential c0/4 (x0^2 - 1)^2 of the cell's origin
ALLENCAHN3 = """const T a0 = x[1] - x[0], a1 = x[3] - x[2], a2 = x[5] - x[4], a3 = x[7] - x[6];
const T b0 = x[2] - x[0], b1 = x[3] - x[1], b2 = x[6] - x[4], b3 = x[7] - x[5];
const T e0 = x[4] - x[0], e1 = x[5] - x[1], e2 = x[6] - x[2], e3 = x[7] - x[3];
const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = T(-0.25) * ((a0 + b0) + e0) + (T(4) * k) * (u * x[0]);
g[1] = T(0.25) * ((a0 - b1) - e1);
g[2] = T(0.25) * ((b0 - a1) - e2);
g[3] = T(0.25) * ((a1 + b1) - e3);
g[4] = T(0.25) * ((e0 - a2) - b2);
g[5] = T(0.25) * ((a2 + e1) - b3);
g[6] = T(0.25) * ((b2 + e2) - a3);
g[7] = T(0.25) * ((a3 + b3) + e3);
const T sa = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
const T sb = (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
const T se = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
return T(0.125) * ((sa + sb) + se) + k * (u * u);"""

# a cell that ignores the slab below: grid_ref.ASYM4's shape on slots 0..3, weighted by p0 at the cell's origin.  As a volume
# objective on (slabs, rows, cols) with p0 zero on the last slab and on the last row of every slab it is SLAB_GRID_2D as a
# grid objective on (slabs*rows, cols): the grid's extra cells, which straddle two slabs, start on a last row and are zero
_SLAB_GRID = """const T s = ((x[0] + T(2) * x[1]) + T(3) * x[2]) + T(5) * x[3];
const T q = p0[i] * s;
g[0] = q;
g[1] = T(2) * q;
g[2] = T(3) * q;
g[3] = T(5) * q;
"""
SLAB_GRID_2D = _SLAB_GRID + "return T(0.5) * (q * s);"
SLAB_GRID = _SLAB_GRID + "g[4] = T(0);\ng[5] = T(0);\ng[6] = T(0);\ng[7] = T(0);\nreturn T(0.5) * (q * s);"


def corners(a, slabs, rows, cols):
    """the eight (slabs-1) x (rows-1) x (cols-1) views of a flat per-node array: slots 0..7 of every cell"""
    A = a.reshape(slabs, rows, cols)
    return [A[ds:slabs - 1 + ds, dr:rows - 1 + dr, dc:cols - 1 + dc] for ds in (0, 1) for dr in (0, 1) for dc in (0, 1)]


def asym8_terms(x, slabs, rows, cols, p0, scalars=ASYM_SCALARS):
    dt = x.dtype.type
    x0, x1, x2, x3, x4, x5, x6, x7 = corners(x, slabs, rows, cols)
    w0, w1, w2, w3, w4, w5, w6, w7 = corners(p0, slabs, rows, cols)
    c0, c1, c2 = dt(scalars[0]), dt(scalars[1]), dt(scalars[2])
    slab = np.arange(slabs - 1).astype(x.dtype)[:, None, None]
    row = np.arange(rows - 1).astype(x.dtype)[None, :, None]
    col = np.arange(cols - 1).astype(x.dtype)[None, None, :]
    s0 = ((w0 * x0 + dt(2) * (w1 * x1)) + dt(3) * (w2 * x2)) + dt(5) * (w3 * x3)
    s1 = ((dt(7) * (w4 * x4) + dt(11) * (w5 * x5)) + dt(13) * (w6 * x6)) + dt(17) * (w7 * x7)
    q = (s0 + s1) + ((slab * c0 + row * c1) + col * c2)
    tg = [w0 * q, dt(2) * (w1 * q), dt(3) * (w2 * q), dt(5) * (w3 * q), dt(7) * (w4 * q), dt(11) * (w5 * q), dt(13) * (w6 * q),
          dt(17) * (w7 * q)]
    return tg, dt(0.5) * (q * q)


def allencahn3_terms(x, slabs, rows, cols, c0):
    dt = x.dtype.type
    x0, x1, x2, x3, x4, x5, x6, x7 = corners(x, slabs, rows, cols)
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


def slab_grid_terms(x, slabs, rows, cols, p0):
    dt = x.dtype.type
    x0, x1, x2, x3 = corners(x, slabs, rows, cols)[:4]
    w = corners(p0, slabs, rows, cols)[0]
    s = ((x0 + dt(2) * x1) + dt(3) * x2) + dt(5) * x3
    q = w * s
    z = np.zeros_like(q)
    return [q, dt(2) * q, dt(3) * q, dt(5) * q, z, z, z, z], dt(0.5) * (q * s)


# slot 7 of cell (s-1, r-1, c-1) ... slot 0 of cell (s, r, c): ascending flat index of the cell's origin
ORDER = tuple((7 - q, (1 - (q >> 2 & 1), 1 - (q >> 1 & 1), 1 - (q & 1))) for q in range(8))


def volume_grad(tg, slabs, rows, cols):
    """flat gradient: per node the contributions of the up to eight cells it is a corner of, ascending cell origin, no leading
    0 +"""
    dt = tg[0].dtype
    shape = (slabs, rows, cols)
    assert min(shape) >= 2 and all(a.shape == (slabs - 1, rows - 1, cols - 1) and a.dtype == dt for a in tg)
    g = np.zeros(shape, dt)
    has = np.zeros(shape, bool)
    for slot, (ds, dr, dc) in ORDER:
        c = np.zeros(shape, dt)
        valid = np.zeros(shape, bool)
        c[ds:ds + slabs - 1, dr:dr + rows - 1, dc:dc + cols - 1] = tg[slot]
        valid[ds:ds + slabs - 1, dr:dr + rows - 1, dc:dc + cols - 1] = True
        g = np.where(valid, np.where(has, g + c, c), g)
        has |= valid
    assert has.all() and g.dtype == dt
    return g.reshape(-1)


def volume_grad_scalar(tg, slabs, rows, cols):
    """the same rule as a plain loop over the nodes (the proof of volume_grad)"""
    dt = tg[0].dtype.type
    g = np.zeros(slabs * rows * cols, tg[0].dtype)
    for s in range(slabs):
        for r in range(rows):
            for c in range(cols):
                acc = None
                for slot, (ds, dr, dc) in ORDER:
                    cs, cr, cc = s - ds, r - dr, c - dc
                    if 0 <= cs < slabs - 1 and 0 <= cr < rows - 1 and 0 <= cc < cols - 1:
                        v = tg[slot][cs, cr, cc]
                        acc = v if acc is None else dt(acc + v)
                g[(s * rows + r) * cols + c] = acc
    return g
