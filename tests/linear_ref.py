"""The numpy restatement of a linear-model objective (include/lbfgsx.h, "linear-model objectives"; csrc/linear_kernels.cuh,
csrc/linear_topology.hip), one numpy operation per source operation, in the element type of the arrays it is given:

    f(x) = sum_j psi(x[j]; j) + sum_r phi(z_r; r),      z = A x,  A in CSR (rowptr, col, val)

  * row_sums: z for L lanes per row -- lane l sums the products of the row's entries k0+l, k0+l+L, .. in ascending order from
    its first one (+0 without one), then s_l = s_l + s_{l+h} for l < h, h = L/2 .. 1;
  * transpose: the stable sort of the CSR entries by column (colptr, the row of every entry, the CSR position it came from);
  * chunk_table: the columns with more than C entries and their chunks of C consecutive entries;
  * gradient: per column psi's derivative, then val * w[row] over the column's entries in list order, started from the first
    contribution; a long column adds its chunk partials instead (256 threads per chunk, strided sums, then halving);
  * the bodies the tests compile, and their numpy twins.
The matrices of the tests are here too."""
import numpy as np

C_DEFAULT = 4096  # kLinearChunk
TRIAL_U = 2       # kLinTrialU: the tile depth of the two trial column kernels

# ---- bodies: + - * /, compare and select only
# an asymmetric cubic phi(u) = u^3 + u^2 + u/2 of u = z - p0[r]
CUBIC = """
const T u = z - p0[r];
dz = (T(3) * u + T(2)) * u + T(0.5);
return ((u + T(1)) * u + T(0.5)) * u;"""
# the squared hinge max(0, 1 - y z)^2 with the label y = p0[r]
HINGE = """
const T m = T(1) - p0[r] * z;
const T h = m > T(0) ? m : T(0);
dz = T(-2) * (p0[r] * h);
return h * h;"""
# least squares 1/2 (z - p0[r])^2
SQUARE = """
const T u = z - p0[r];
dz = u;
return T(0.5) * (u * u);"""
# logistic loss log(1 + exp(-y z)), y = p0[r] in {-1, +1}, in the overflow-free form
LOGISTIC = """
const T m = p0[r] * z;
const T e = exp(T(0) - fabs(m));
const T s = (m > T(0) ? e : T(1)) / (T(1) + e);
dz = T(0) - p0[r] * s;
return (m > T(0) ? T(0) : T(0) - m) + log1p(e);"""
# the ridge c[0]/2 x^2 per coordinate
RIDGE = """
g[0] = c[0] * x[0];
return T(0.5) * (c[0] * (x[0] * x[0]));"""


def cubic(z, p0):
    dt = z.dtype.type
    u = z - p0
    return (dt(3) * u + dt(2)) * u + dt(0.5), ((u + dt(1)) * u + dt(0.5)) * u


def hinge(z, p0):
    dt = z.dtype.type
    m = dt(1) - p0 * z
    h = np.where(m > dt(0), m, dt(0)).astype(z.dtype)
    return dt(-2) * (p0 * h), h * h


def ridge(x, c0):
    dt = x.dtype.type
    c0 = dt(c0)
    return c0 * x, dt(0.5) * (c0 * (x * x))


ROW_BODIES = {"cubic": (CUBIC, cubic), "hinge": (HINGE, hinge)}


# ---- the semantics
def lanes_rule(R, nnz):
    """the largest power of two <= max(1, nnz // R), at most 64"""
    L = 1
    while L < 64 and 2 * L <= nnz // R:
        L *= 2
    return L


def _halve(S):
    """s_l = s_l + s_{l+h} for l < h, h = width/2 .. 1, along the last axis; returns s_0"""
    h = S.shape[-1] // 2
    while h >= 1:
        S[..., :h] = S[..., :h] + S[..., h:2 * h]
        h //= 2
    return S[..., 0]


def row_sums(rowptr, col, val, x, L):
    rowptr = np.asarray(rowptr, np.int64)
    R = rowptr.size - 1
    S = np.zeros((R, L), x.dtype)
    lens = np.diff(rowptr)
    lane = np.arange(L, dtype=np.int64)[None, :]
    for i in range(int(-(-int(lens.max()) // L)) if R else 0):
        K = rowptr[:-1, None] + lane + i * L
        ok = K < rowptr[1:, None]
        prod = val[K[ok]] * x[col[K[ok]]]
        S[ok] = prod if i == 0 else S[ok] + prod
    return _halve(S)


def transpose(rowptr, col, n):
    """colptr (n+1, uint32), trow and tpos (nnz): the CSR entries in a stable order by column"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    tpos = np.argsort(col, kind="stable")
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    colptr = np.zeros(n + 1, np.int64)
    np.add.at(colptr, col + 1, 1)
    return np.cumsum(colptr).astype(np.uint32), rows[tpos].astype(np.int32), tpos.astype(np.uint32)


def chunk_table(colptr, C=C_DEFAULT):
    """long_col (int32), long_chunk (uint32, one more than long columns), chunk (uint32, (chunks, 2): first, past-the-last)"""
    colptr = np.asarray(colptr, np.int64)
    long_col = np.flatnonzero(np.diff(colptr) > C)
    long_chunk, chunk = [0], []
    for j in long_col:
        for b in range(int(colptr[j]), int(colptr[j + 1]), C):
            chunk.append((b, min(b + C, int(colptr[j + 1]))))
        long_chunk.append(len(chunk))
    return long_col.astype(np.int32), np.asarray(long_chunk, np.uint32), np.asarray(chunk, np.uint32).reshape(-1, 2)


def chunk_partial(prod, width=256):
    """thread t of `width` sums prod[t], prod[t + width], .. from its first (+0 without one), then the halving"""
    S = np.zeros(width, prod.dtype)
    for i in range(0, prod.size, width):
        seg = prod[i:i + width]
        S[:seg.size] = seg if i == 0 else S[:seg.size] + seg
    return _halve(S)


def gradient(w, val, topo, n, C=C_DEFAULT, psi_g=None):
    """grad[j]: psi_g[j] if given, then the contributions of column j in list order, from the first one"""
    colptr, trow, tpos = topo
    colptr = colptr.astype(np.int64)
    prod = val[tpos] * w[trow]
    g = np.zeros(n, w.dtype) if psi_g is None else psi_g.copy()
    has = np.zeros(n, bool) if psi_g is None else np.ones(n, bool)
    lens = np.diff(colptr)
    short = lens <= C
    for k in range(int(lens[short].max()) if short.any() else 0):
        js = np.flatnonzero(short & (lens > k))
        p = prod[colptr[js] + k]
        g[js] = np.where(has[js], g[js] + p, p)
        has[js] = True
    for j in np.flatnonzero(~short):
        for b in range(int(colptr[j]), int(colptr[j + 1]), C):
            p = chunk_partial(prod[b:min(b + C, int(colptr[j + 1]))])
            g[j] = g[j] + p if has[j] else p
            has[j] = True
    return g


class Problem:
    """one matrix with per-row data p0 and the ridge weight c0; evaluate(x, L, row, with_ridge) -> (g, all term values)"""

    def __init__(self, rowptr, col, val, n, p0, c0=0.25, C=C_DEFAULT):
        self.rowptr, self.col = np.asarray(rowptr, np.int32), np.asarray(col, np.int32)
        self.val, self.p0, self.n, self.c0, self.C = val, p0, n, c0, C
        self.R, self.nnz = self.rowptr.size - 1, self.col.size
        self.topo = transpose(self.rowptr, self.col, n)
        self._z = {}

    def z(self, x, L):
        key = (x.tobytes(), L)
        if key not in self._z:
            self._z[key] = row_sums(self.rowptr, self.col, self.val, x, L)
        return self._z[key]

    def evaluate(self, x, L, row, with_ridge):
        w, v = ROW_BODIES[row][1](self.z(x, L), self.p0)
        if not with_ridge:
            return gradient(w, self.val, self.topo, self.n, self.C), v
        pg, pv = ridge(x, self.c0)
        return gradient(w, self.val, self.topo, self.n, self.C, pg), np.concatenate([v, pv])

    def has_long(self):
        return bool((np.diff(self.topo[0].astype(np.int64)) > self.C).any())


# ---- the matrices of the tests
def _csr(rows, n, rng, dt):
    """rows: per row the list of its column indices, in the order given"""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.asarray([c for r in rows for c in r], np.int32)
    val = rng.standard_normal(col.size).astype(dt)
    p0 = np.where(rng.random(len(rows)) < 0.5, -1.0, 1.0).astype(dt) * (0.5 + rng.random(len(rows))).astype(dt)
    return Problem(rowptr, col, val, n, p0)


def single(dt):
    return _csr([[0]], 1, np.random.default_rng(1), dt)


def tiny(dt):
    """R = 3, n = 5: row 1 is empty, column 2 is empty, (0, 3) is listed twice, and row 2 is not sorted by column"""
    return _csr([[3, 0, 3], [], [4, 1, 0]], 5, np.random.default_rng(2), dt)


def random_rows(R, n, maxlen, seed, dt):
    """row lengths 0 .. maxlen, columns drawn with replacement (duplicates occur) in random order"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, R)
    lens[0] = 0
    lens[R // 2] = maxlen
    return _csr([list(rng.integers(0, n, k)) for k in lens], n, rng, dt)


def long_columns(dt, R=9000, n=37, C=C_DEFAULT):
    """column 0 dense (an intercept), column 5 with exactly C entries, column n - 1 (a tail coordinate) with C + 1, the rest
    sparse"""
    rng = np.random.default_rng(3)
    in5, in36 = set(rng.choice(R, C, replace=False).tolist()), set(rng.choice(R, C + 1, replace=False).tolist())
    rows = []
    for r in range(R):
        cs = [0]
        if r in in36:
            cs.append(n - 1)
        if r in in5:
            cs.append(5)
        cs += [int(c) for c in rng.integers(1, n - 1, rng.integers(0, 3)) if c != 5]
        rows.append(cs)
    P = _csr(rows, n, rng, dt)
    P.C = C
    return P
