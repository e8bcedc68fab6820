"""Grid objectives (lbfgspp_amd.GridObjective, csrc/grid_kernels.cuh): the bodies the tests compile and their plain numpy
restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x is a row-major rows x cols array.  A restatement returns (tg, v): tg[j][r, c] the j-th partial derivative of cell (r, c) --
slots 0..3 are the nodes (r, c), (r, c+1), (r+1, c), (r+1, c+1) -- and v[r, c] its value, for 0 <= r < rows-1, 0 <= c < cols-1.
grid_grad puts the gradient together by the rule of include/lbfgsx.h: grad[r, c] = tg[3][r-1, c-1] + tg[2][r-1, c] +
tg[1][r, c-1] + tg[0][r, c], the cells that exist, in this order, started from the first.  The bodies use + - * only."""
import numpy as np

# the statement tests' body: another weight on each slot and each partial, p0 read at all four corners, row and col in the value
#   q = w0 x0 + 2 w1 x1 + 3 w2 x2 + 5 w3 x3 + (row c0 + col c1),  value q^2 / 2
ASYM4 = """const T w0 = p0[i], w1 = p0[i + 1], w2 = p0[i + cols], w3 = p0[i + cols + 1];
const T s = ((w0 * x[0] + T(2) * (w1 * x[1])) + T(3) * (w2 * x[2])) + T(5) * (w3 * x[3]);
const T q = s + (T(row) * c[0] + T(col) * c[1]);
g[0] = w0 * q;
g[1] = T(2) * (w1 * q);
g[2] = T(3) * (w2 * q);
g[3] = T(5) * (w3 * q);
return T(0.5) * (q * q);"""
ASYM_SCALARS = (0.3, -0.7)  # c0, c1: neither is a float or a double

# Allen-Cahn: the squared differences along the cell's four edges, each with half its weight (an inner edge belongs to two
# cells), plus the double-well potential c0/4 (x0^2 - 1)^2 of the cell's origin
ALLENCAHN = """const T a = x[1] - x[0];
const T b = x[2] - x[0];
const T e = x[3] - x[2];
const T h = x[3] - x[1];
const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[0]);
g[1] = T(0.5) * (a - h);
g[2] = T(0.5) * (b - e);
g[3] = T(0.5) * (e + h);
return T(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u);"""

# a row-wise pair term that ignores the row below: as a grid objective and, without its last line, as a K = 2 chain
ROW_PAIR_CHAIN = """const T u = x[1] - x[0] * x[0];
const T pu = p0[i] * u;
g[1] = T(2) * pu;
g[0] = T(-4) * (pu * x[0]);
"""
ROW_PAIR_GRID = ROW_PAIR_CHAIN + "g[2] = T(0);\ng[3] = T(0);\nreturn pu * u;"
ROW_PAIR_CHAIN += "return pu * u;"


def corners(a, rows, cols):
    """the four (rows-1) x (cols-1) views of a flat per-node array: slots 0..3 of every cell"""
    A = a.reshape(rows, cols)
    return A[:-1, :-1], A[:-1, 1:], A[1:, :-1], A[1:, 1:]


def asym4_terms(x, rows, cols, p0, scalars=ASYM_SCALARS):
    dt = x.dtype.type
    x0, x1, x2, x3 = corners(x, rows, cols)
    w0, w1, w2, w3 = corners(p0, rows, cols)
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    row = np.arange(rows - 1).astype(x.dtype)[:, None]
    col = np.arange(cols - 1).astype(x.dtype)[None, :]
    s = ((w0 * x0 + dt(2) * (w1 * x1)) + dt(3) * (w2 * x2)) + dt(5) * (w3 * x3)
    q = s + (row * c0 + col * c1)
    return [w0 * q, dt(2) * (w1 * q), dt(3) * (w2 * q), dt(5) * (w3 * q)], dt(0.5) * (q * q)


def allencahn_terms(x, rows, cols, c0):
    dt = x.dtype.type
    x0, x1, x2, x3 = corners(x, rows, cols)
    a = x1 - x0
    b = x2 - x0
    e = x3 - x2
    h = x3 - x1
    u = x0 * x0 - dt(1)
    k = dt(c0) * dt(0.25)
    tg = [dt(-0.5) * (a + b) + (dt(4) * k) * (u * x0), dt(0.5) * (a - h), dt(0.5) * (b - e), dt(0.5) * (e + h)]
    return tg, dt(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u)


def grid_grad(tg, rows, cols):
    """flat gradient: per node the contributions of the up to four cells it is a corner of, ascending cell origin, no leading 0 +"""
    dt = tg[0].dtype
    assert rows >= 2 and cols >= 2 and all(a.shape == (rows - 1, cols - 1) and a.dtype == dt for a in tg)
    g = np.zeros((rows, cols), dt)
    has = np.zeros((rows, cols), bool)
    # slot 3 of cell (r-1, c-1), slot 2 of cell (r-1, c), slot 1 of cell (r, c-1), slot 0 of cell (r, c)
    for slot, (dr, dc) in ((3, (1, 1)), (2, (1, 0)), (1, (0, 1)), (0, (0, 0))):
        c = np.zeros((rows, cols), dt)
        valid = np.zeros((rows, cols), bool)
        c[dr:dr + rows - 1, dc:dc + cols - 1] = tg[slot]
        valid[dr:dr + rows - 1, dc:dc + cols - 1] = True
        g = np.where(valid, np.where(has, g + c, c), g)
        has |= valid
    assert has.all() and g.dtype == dt
    return g.reshape(-1)


def grid_grad_scalar(tg, rows, cols):
    """the same rule as a plain loop over the nodes (the proof of grid_grad)"""
    dt = tg[0].dtype.type
    g = np.zeros(rows * cols, tg[0].dtype)
    for r in range(rows):
        for c in range(cols):
            acc = None
            for slot, (cr, cc) in ((3, (r - 1, c - 1)), (2, (r - 1, c)), (1, (r, c - 1)), (0, (r, c))):
                if 0 <= cr < rows - 1 and 0 <= cc < cols - 1:
                    v = tg[slot][cr, cc]
                    acc = v if acc is None else dt(acc + v)
            g[r * cols + c] = acc
    return g
