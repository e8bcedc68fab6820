"""The numpy restatement of a dense linear-model objective (include/lbfgsx.h, "dense linear-model objectives";
csrc/linear_dense_kernels.cuh), one numpy operation per source operation, in the element type of the arrays it is given:

    x = X (F x D, feature-major: x[j*D + c]),   A dense R x F,   Z = A X,   f(x) = sum_i psi(x[i]; i) + sum_r phi(Z[r, 0..D); r)

  * row_sums: Z for L lanes per row -- per output c, lane l sums A[r,k]*X[k, c] over the columns l, l+L, .. in ascending order
    from its first one (+0 without one), then s_l = s_l + s_{l+h} for l < h, h = L/2 .. 1;
  * partials: rows cut into chunks of C consecutive rows; part[b, j, c] = the sum over the rows r of chunk b, ascending, of
    A[r,j]*W[r,c], started from the first product;
  * gradient: psi's derivative if given, then the partials in ascending b, started from the first contribution.
L, C and D are parameters.  The bodies and their numpy twins are tests/multilinear_ref.py's (the two forms share their
bodies' signatures); nothing of the library is imported."""
import numpy as np

import linear_ref as LR
import multilinear_ref as MR

C_DEFAULT = 256   # kDenseChunk
TRIAL_U = LR.TRIAL_U
BLOCK = 256       # kBlock


def lanes_rule(F):
    """the largest power of two <= F, at most 64: the sparse rule with nnz / R = F"""
    return LR.lanes_rule(1, F)


def row_sums(Amat, X, L):
    """Z (R x D) from X (F x D)"""
    R, F = Amat.shape
    D = X.shape[1]
    S = np.zeros((R, D, L), X.dtype)
    for i in range(-(-F // L)):
        k = np.arange(i * L, min(F, (i + 1) * L))            # lane l = k - i*L takes column k
        prod = Amat[:, k, None] * X[None, k, :]               # (R, lanes, D)
        prod = np.transpose(prod, (0, 2, 1))
        S[:, :, :k.size] = prod if i == 0 else S[:, :, :k.size] + prod
    return LR._halve(S)


def partials(Amat, W, C=C_DEFAULT):
    """part (chunks x F x D)"""
    R, F = Amat.shape
    D = W.shape[1]
    chunks = -(-R // C)
    part = np.zeros((chunks, F, D), W.dtype)
    for b in range(chunks):
        for t, r in enumerate(range(b * C, min(R, (b + 1) * C))):
            prod = Amat[r][:, None] * W[r][None, :]
            part[b] = prod if t == 0 else part[b] + prod
    return part


def gradient(part, psi_g=None):
    """grad (F x D): psi_g if given, then the chunk partials in ascending order, from the first contribution"""
    g = None if psi_g is None else psi_g.copy()
    for b in range(part.shape[0]):
        g = part[b].copy() if g is None else g + part[b]
    return g


def softmax(Z, p0, c1):
    """the numpy twin of the softmax cross-entropy body (test_multilinear_objective_cpu.SOFTMAX), operation for operation;
    exp and log are the platform's, which need not round as the device's do"""
    dt = Z.dtype.type
    R, D = Z.shape
    y = p0.astype(np.int64)
    m = Z[:, 0].copy()
    for k in range(1, D):
        m = np.where(Z[:, k] > m, Z[:, k], m)
    E = np.empty_like(Z)
    s = np.zeros(R, Z.dtype)
    for k in range(D):
        E[:, k] = np.exp(Z[:, k] - m)
        s = s + E[:, k]
    zy = Z[:, 0].copy()
    for k in range(1, D):
        zy = np.where(y == k, Z[:, k], zy)
    W = np.empty_like(Z)
    for k in range(D):
        W[:, k] = dt(c1) * (E[:, k] / s - np.where(y == k, dt(1), dt(0)))
    return W, dt(c1) * ((np.log(s) + m) - zy)


class Problem:
    """a dense R x F matrix (row stride lda >= F: Astore[:, :F] is A) with D outputs: targets (R*D, the coupled body's p0),
    labels (R, the hinge's p0), the ridge weight c0 and the coupling c1; evaluate(x, L, row, with_ridge) ->
    (g of n = F*D, all term values, W, v, part)"""

    def __init__(self, R, F, D, dt, seed=0, pad=0, C=C_DEFAULT):
        rng = np.random.default_rng(2000 + seed)
        self.R, self.F, self.D, self.n, self.C, self.lda = R, F, D, F * D, C, F + pad
        self.Astore = np.full((R, F + pad), -9.0, dt)  # the padding is never read: were it, every sum would show it
        self.Astore[:, :F] = rng.standard_normal((R, F)).astype(dt)
        self.A = self.Astore[:, :F]
        self.targets = rng.standard_normal(R * D).astype(dt)
        self.labels = rng.integers(0, D, R).astype(dt)
        self.c0, self.c1 = 0.25, 0.125
        self.chunks = -(-R // C)
        self._z = {}

    def p0(self, row):
        return self.targets if row == "coupled" else self.labels

    def z(self, x, L):
        key = (x.tobytes(), L)
        if key not in self._z:
            self._z[key] = row_sums(self.A, x.reshape(self.F, self.D), L)
        return self._z[key]

    def evaluate(self, x, L, row, with_ridge):
        W, v = MR.ROW_BODIES[row][1](self.z(x, L), self.p0(row), self.c1)
        part = partials(self.A, W, self.C)
        if not with_ridge:
            return gradient(part).reshape(-1), v, W, v, part
        pg, pv = LR.ridge(x, self.c0)
        return gradient(part, pg.reshape(self.F, self.D)).reshape(-1), np.concatenate([v, pv]), W, v, part

    def csr(self):
        """the same matrix as CSR with every entry stored"""
        rowptr = np.arange(0, self.R * self.F + 1, self.F, dtype=np.int64)
        col = np.tile(np.arange(self.F, dtype=np.int64), self.R)
        return rowptr, col, np.ascontiguousarray(self.A).reshape(-1)


# name -> (R, F, D, pad): the smallest shapes at which each pass can go wrong (R <= 800, F <= 300).  W = 2 (f64) or 4 (f32)
# columns per thread in the partial pass and coordinates per thread in the column pass; L = min(64, pow2 <= F) lanes per row
# and 256 / L rows per block step in the row pass; C = 256 rows per chunk.
SHAPES = {
    "f1":      (1, 1, 1, 0),       # F = 1, R = 1: one lane, one chunk of one row, n = 1 (all tail)
    "f3":      (255, 3, 3, 0),     # F = 3 < W in f32, L = 2 with a lane that gets a second column; R = C - 1; D = 3: n = 9, packs
                                   # of coordinates that straddle two features and a tail
    "f64":     (256, 64, 2, 0),    # F = 64 = one full wavefront per row; R = C exactly
    "f65":     (257, 65, 5, 0),    # F = 65: lane 0 alone takes a second column; R = C + 1: a chunk of one row; D = 5
    "f257":    (549, 257, 1, 0),   # F = 257: past one load group of 64 lanes (4 in flight), odd; R = 2*256 + 37; D = 1
    "pad":     (300, 37, 2, 3),    # lda = F + 3: rows not aligned to 16 bytes, element loads in the partial pass
    "wide16":  (130, 20, 16, 0),   # D = 16: whole packs per weight row, one column in flight per lane; R not a multiple of
                                   # 256 / L = 16
    "ntail":   (70, 7, 3, 0),      # n = 21: not a multiple of W in either dtype (thread 0 of block 0's tail)
    "big":     (800, 300, 8, 0),   # 150 packs in f64 (S = 256), 75 in f32 (S = 128: two chunks per block), 4 chunks; n = 2400:
                                   # past one trial tile of the column pass in both dtypes
}


def problem(name, dt, C=C_DEFAULT):
    R, F, D, pad = SHAPES[name]
    return Problem(R, F, D, dt, seed=sorted(SHAPES).index(name), pad=pad, C=C)
