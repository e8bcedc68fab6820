"""The numpy restatement of a multi-output linear-model objective (include/lbfgsx.h, "multi-output linear-model objectives";
csrc/linear_multi_kernels.cuh, csrc/linear_topology.hip), one numpy operation per source operation, in the element type of
the arrays it is given:

    x = X (F x D, feature-major: x[j*D + c]),   Z = A X,   f(x) = sum_i psi(x[i]; i) + sum_r phi(Z[r, 0..D); r)

  * row_sums: Z for L lanes per row -- per output c, lane l sums val[k]*X[col[k], c] over the row's entries k0+l, k0+l+L, .. in
    ascending order from its first one (+0 without one), then s_l = s_l + s_{l+h} for l < h, h = L/2 .. 1;
  * gradient: per coordinate (j, c) psi's derivative, then val * W[row, c] over column j's entries in list order, started from
    the first contribution; a long column adds its chunk partials per output instead (256 threads per chunk and output);
  * the bodies the tests compile, and their numpy twins.
The transposed list, the chunk table, the lane rule and the matrices are tests/linear_ref.py's (the matrix is R x F whatever
D is); nothing of the library is imported."""
import numpy as np

import linear_ref as LR

C_DEFAULT = LR.C_DEFAULT
TRIAL_U = LR.TRIAL_U

# ---- bodies: + - * /, compare and select only (loop variables are not called c: c[8] are the scalars)
# coupled least squares: phi = 1/2 sum_k (z_k - p0[r*D + k])^2 + c[1] (sum_k z_k)^2
COUPLED = """
T t = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    t = t + z[k];
T u[D];
T q = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    u[k] = z[k] - p0[r * D + k];
    q = q + u[k] * u[k];
}
#pragma unroll
for (int k = 0; k < D; k++)
    dz[k] = u[k] + T(2) * (c[1] * t);
return T(0.5) * q + c[1] * (t * t);"""
# the multi-class squared hinge with the label y = int(p0[r]): phi = sum_{k != y} max(0, (1 + z_k) - z_y)^2
MHINGE = """
const int y = int(p0[r]);
T zy = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    zy = k == y ? z[k] : zy;
T v = T(0), sd = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    const T m = (T(1) + z[k]) - zy;
    const T h = (k != y && m > T(0)) ? m : T(0);
    const T h2 = T(2) * h;
    dz[k] = h2;
    v = v + h * h;
    sd = sd + h2;
}
#pragma unroll
for (int k = 0; k < D; k++)
    dz[k] = k == y ? T(0) - sd : dz[k];
return v;"""
RIDGE = LR.RIDGE
# the D = 1 twins of linear_ref's bodies in the multi-output signature
def scalar_body(body):
    return "const T zz = z[0]; T dd = T(0); const T value = [&](const T z, T& dz) {%s\n}(zz, dd); dz[0] = dd; return value;" % body


def coupled(Z, p0, c1):
    dt = Z.dtype.type
    D = Z.shape[1]
    t = Z[:, 0].copy()
    for k in range(1, D):
        t = t + Z[:, k]
    U = np.empty_like(Z)
    q = np.zeros(Z.shape[0], Z.dtype)
    T_ = p0.reshape(-1, D)
    for k in range(D):
        U[:, k] = Z[:, k] - T_[:, k]
        q = q + U[:, k] * U[:, k]
    W = np.empty_like(Z)
    for k in range(D):
        W[:, k] = U[:, k] + dt(2) * (dt(c1) * t)
    return W, dt(0.5) * q + dt(c1) * (t * t)


def mhinge(Z, p0, c1=None):
    dt = Z.dtype.type
    R, D = Z.shape
    y = p0.astype(np.int64)
    zy = Z[:, 0].copy()
    for k in range(1, D):
        zy = np.where(y == k, Z[:, k], zy)
    v, sd = np.zeros(R, Z.dtype), np.zeros(R, Z.dtype)
    W = np.empty_like(Z)
    for k in range(D):
        m = (dt(1) + Z[:, k]) - zy
        h = np.where((y != k) & (m > dt(0)), m, dt(0)).astype(Z.dtype)
        h2 = dt(2) * h
        W[:, k] = h2
        v = v + h * h
        sd = sd + h2
    for k in range(D):
        W[:, k] = np.where(y == k, dt(0) - sd, W[:, k])
    return W, v


ROW_BODIES = {"coupled": (COUPLED, coupled), "mhinge": (MHINGE, mhinge)}


# ---- the semantics
def row_sums(rowptr, col, val, X, L):
    """Z (R x D) from X (F x D)"""
    rowptr = np.asarray(rowptr, np.int64)
    R, D = rowptr.size - 1, X.shape[1]
    S = np.zeros((R, D, L), X.dtype)
    lens = np.diff(rowptr)
    lane = np.arange(L, dtype=np.int64)[None, :]
    for i in range(int(-(-int(lens.max()) // L)) if R else 0):
        K = rowptr[:-1, None] + lane + i * L
        ok = K < rowptr[1:, None]
        rr, ll = np.nonzero(ok)
        prod = val[K[ok]][:, None] * X[col[K[ok]]]  # (entries, D)
        S[rr, :, ll] = prod if i == 0 else S[rr, :, ll] + prod
    return LR._halve(S)


def chunk_partial(prod, width=256):
    """per output: thread t of `width` sums prod[t], prod[t + width], .. from its first (+0 without one), then the halving"""
    S = np.zeros((prod.shape[1], width), prod.dtype)
    for i in range(0, prod.shape[0], width):
        seg = prod[i:i + width].T
        S[:, :seg.shape[1]] = seg if i == 0 else S[:, :seg.shape[1]] + seg
    return LR._halve(S)


def gradient(W, val, topo, F, C=C_DEFAULT, psi_g=None):
    """grad (F x D): psi_g if given, then the contributions of column j in list order, from the first one"""
    colptr, trow, tpos = topo
    colptr = colptr.astype(np.int64)
    D = W.shape[1]
    prod = val[tpos][:, None] * W[trow]
    g = np.zeros((F, D), W.dtype) if psi_g is None else psi_g.copy()
    has = np.zeros(F, bool) if psi_g is None else np.ones(F, bool)
    lens = np.diff(colptr)
    short = lens <= C
    for k in range(int(lens[short].max()) if short.any() else 0):
        js = np.flatnonzero(short & (lens > k))
        p = prod[colptr[js] + k]
        g[js] = np.where(has[js][:, None], g[js] + p, p)
        has[js] = True
    for j in np.flatnonzero(~short):
        for b in range(int(colptr[j]), int(colptr[j + 1]), C):
            p = chunk_partial(prod[b:min(b + C, int(colptr[j + 1]))])
            g[j] = g[j] + p if has[j] else p
            has[j] = True
    return g


class Problem:
    """a matrix of tests/linear_ref.py (R x F) with D outputs: targets (R*D, the coupled body's p0), labels (R, the hinge's
    p0), the ridge weight c0 and the coupling c1; evaluate(x, L, row, with_ridge) -> (g of n = F*D, all term values)"""

    def __init__(self, P, D, seed=0):
        rng = np.random.default_rng(1000 + seed)
        dt = P.val.dtype
        self.P, self.D, self.F, self.n = P, D, P.n, P.n * D
        self.rowptr, self.col, self.val, self.R, self.nnz, self.topo, self.C = P.rowptr, P.col, P.val, P.R, P.nnz, P.topo, P.C
        self.targets = rng.standard_normal(P.R * D).astype(dt)
        self.labels = rng.integers(0, D, P.R).astype(dt)
        self.c0, self.c1 = 0.25, 0.125
        self._z = {}

    def p0(self, row):
        return self.targets if row == "coupled" else self.labels

    def z(self, x, L):
        key = (x.tobytes(), L)
        if key not in self._z:
            self._z[key] = row_sums(self.rowptr, self.col, self.val, x.reshape(self.F, self.D), L)
        return self._z[key]

    def evaluate(self, x, L, row, with_ridge):
        W, v = ROW_BODIES[row][1](self.z(x, L), self.p0(row), self.c1)
        if not with_ridge:
            return gradient(W, self.val, self.topo, self.F, self.C).reshape(-1), v
        pg, pv = LR.ridge(x, self.c0)
        return gradient(W, self.val, self.topo, self.F, self.C, pg.reshape(self.F, self.D)).reshape(-1), np.concatenate([v, pv])

    def has_long(self):
        return self.P.has_long()


# ---- the matrices of the tests
def fixed_rows(R, F, per, seed, dt):
    """exactly `per` entries per row, columns drawn with replacement in random order"""
    rng = np.random.default_rng(seed)
    return LR._csr([list(rng.integers(0, F, per)) for _ in range(R)], F, rng, dt)


def problem(name, dt):
    """the shapes of the statement tests: the smallest at which each path can go wrong"""
    W = 2 if np.dtype(dt) == np.float64 else 4
    if name == "single":   # n = 3: no whole pack in f32
        return Problem(LR.single(dt), 3, 1)
    if name == "tiny":     # n = 15: a ragged tail, packs that straddle two features
        return Problem(LR.tiny(dt), 3, 2)
    if name == "random":   # D = 10, 7 entries per row
        return Problem(fixed_rows(700, 103, 7, 7, dt), 10, 3)
    if name == "wide16":   # D = 16: whole packs per weight row
        return Problem(LR.random_rows(300, 67, 12, 8, dt), 16, 4)
    if name == "tile":     # n one coordinate past one trial tile of the column pass
        F, D = (205, 5) if W == 2 else (683, 3)
        assert F * D == 256 * TRIAL_U * W + 1
        return Problem(LR.random_rows(200, F, 12, 9, dt), D, 5)
    assert name == "long"  # an intercept column: the chunk partials per output
    return Problem(LR.long_columns(dt), 3, 6)
