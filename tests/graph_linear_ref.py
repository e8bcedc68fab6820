"""The numpy restatement of a graph-regularised linear-model objective (include/lbfgsx.h, "graph-regularised linear-model
objectives"; csrc/linear_graph_kernels.cuh), composed from the two restatements it combines, one numpy operation per source
operation, in the element type of the arrays it is given:

    f(x) = sum_j psi(x[j]; j) + sum_e rho(x[ei[e]], x[ej[e]]; e) + sum_r phi(z_r; r),      z = A x

  * z, w and v are linear_ref's (row_sums and the row bodies);
  * grad[j] is ONE sum in a fixed order that starts from its first contribution (+0 without one): psi's derivative if there is a
    coordinate body, then g_e[side] of j's incidence entries in ascending e (graph_ref.incidence), then the column's
    contributions as linear_ref.gradient forms them (the entries in list order, or a long column's chunk partials);
  * the terms of f are every psi value, every edge value and every row value.
The three bodies share p0..p3 and c[8]: the row bodies read p0[r] and the ridge c[0] (linear_ref), so the edge body of the
tests is graph_ref's asymmetric one moved to p2[e], p3[i], p3[j], c[4] and c[5]."""
import numpy as np

import graph_ref as GR
import linear_ref as LR

# graph_ref.ASYM_EDGE beside a row body: its per-edge weight in p2, its per-node weight in p3, its two scalars in c[4], c[5]
ASYM_EDGE = GR.ASYM_EDGE.replace("p0[e]", "p2[e]").replace("p1[i]", "p3[i]").replace("p1[j]", "p3[j]") \
    .replace("c[0]", "c[4]").replace("c[1]", "c[5]")
# graph_ref.SPRING_EDGE with its weight in p2: symmetric in value, antisymmetric in its partials
SPRING_EDGE = GR.SPRING_EDGE.replace("p0[e]", "p2[e]")
EDGE_SCALARS = GR.SCALARS[:2]  # c[4], c[5]
EDGE_BODIES = {"asym": ASYM_EDGE, "spring": SPRING_EDGE}


def edge_terms(name, x, ei, ej, p2, p3):
    """(tg, v) of the named edge body: tg[s][e] the partial of edge e with respect to its end s, v[e] its value"""
    if name == "asym":
        return GR.asym_edge_terms(x, ei, ej, p2, p3, EDGE_SCALARS + (0.0,))
    return GR.spring_terms(x, ei, ej, p2)


def gradient(w, val, topo, ei, ej, n, tg, C=LR.C_DEFAULT, psi_g=None):
    """grad[j]: psi_g[j] if given, then tg[side][e] over j's incidence entries in ascending e, then the column's contributions
    in list order (a long column: its chunk partials in ascending chunk index); from the first one, +0 without one"""
    colptr, trow, tpos = topo
    colptr = colptr.astype(np.int64)
    dt = w.dtype
    g = np.zeros(n, dt) if psi_g is None else psi_g.astype(dt, copy=True)
    has = np.zeros(n, bool) if psi_g is None else np.ones(n, bool)
    # the edges: graph_ref.graph_grad's loop, continued from (g, has)
    off, _, es = GR.incidence(ei, ej, n)
    off = off.astype(np.int64)
    contrib = np.stack([tg[0], tg[1]], 1).reshape(-1)[es.astype(np.int64)]
    deg = np.diff(off)
    for r in range(int(deg.max()) if n else 0):
        idx = np.nonzero(deg > r)[0]
        c = contrib[off[idx] + r]
        g[idx] = np.where(has[idx], g[idx] + c, c)
        has[idx] = True
    # the matrix: linear_ref.gradient's loops, continued from (g, has)
    prod = val[tpos] * w[trow]
    lens = np.diff(colptr)
    short = lens <= C
    for k in range(int(lens[short].max()) if short.any() else 0):
        js = np.flatnonzero(short & (lens > k))
        p = prod[colptr[js] + k]
        g[js] = np.where(has[js], g[js] + p, p)
        has[js] = True
    for j in np.flatnonzero(~short):
        for b in range(int(colptr[j]), int(colptr[j + 1]), C):
            p = LR.chunk_partial(prod[b:min(b + C, int(colptr[j + 1]))])
            g[j] = g[j] + p if has[j] else p
            has[j] = True
    assert g.dtype == dt
    return g


def gradient_scalar(w, val, topo, ei, ej, n, tg, C=LR.C_DEFAULT, psi_g=None):
    """the same rule as plain loops over coordinates, edges and entries (the proof of gradient): graph_ref.graph_grad_scalar's
    walk of the edges, then the column's products or chunk partials, one scalar sum per coordinate"""
    colptr, trow, tpos = topo
    dt = w.dtype.type
    g = np.zeros(n, w.dtype)
    for j in range(n):
        acc = None if psi_g is None else psi_g[j]
        for e in range(len(ei)):
            for side, end in ((0, ei[e]), (1, ej[e])):
                if end == j:
                    acc = tg[side][e] if acc is None else dt(acc + tg[side][e])
        lo, hi = int(colptr[j]), int(colptr[j + 1])
        prod = val[tpos[lo:hi]] * w[trow[lo:hi]]
        if hi - lo > C:
            parts = [LR.chunk_partial(prod[b:b + C]) for b in range(0, hi - lo, C)]
        else:
            parts = list(prod)
        for p in parts:
            acc = p if acc is None else dt(acc + p)
        g[j] = dt(0) if acc is None else acc
    return g


class Problem:
    """a linear_ref.Problem with a graph on its n columns, per-edge data p2 and per-node data p3;
    evaluate(x, L, row, edge, with_ridge) -> (g, all term values)"""

    def __init__(self, P, ei, ej, seed=11):
        self.P, self.n, self.R, self.nnz = P, P.n, P.R, P.nnz
        self.ei, self.ej = np.asarray(ei, np.int32), np.asarray(ej, np.int32)
        self.E = self.ei.size
        rng = np.random.default_rng(seed)
        dt = P.val.dtype
        self.p2 = (0.5 + rng.random(self.E)).astype(dt)
        self.p3 = (rng.standard_normal(self.n) * 0.5).astype(dt)
        self.scalars = (P.c0, 0.0, 0.0, 0.0) + EDGE_SCALARS

    def evaluate(self, x, L, row, edge, with_ridge):
        P = self.P
        w, v = LR.ROW_BODIES[row][1](P.z(x, L), P.p0)
        tg, ev = edge_terms(edge, x, self.ei.astype(np.int64), self.ej.astype(np.int64), self.p2, self.p3)
        pg, pv = LR.ridge(x, P.c0) if with_ridge else (None, np.zeros(0, x.dtype))
        g = gradient(w, P.val, P.topo, self.ei, self.ej, self.n, tg, P.C, pg)
        return g, np.concatenate([pv, ev, v])

    def has_long(self):
        return self.P.has_long()


# ---- the instances of the tests
def pair(dt):
    """n = 2, R = 1, one edge: no whole pack of coordinates"""
    return Problem(LR._csr([[1, 0]], 2, np.random.default_rng(1), dt), [1], [0])


def tiny(dt):
    """linear_ref.tiny (R = 3, n = 5, column 2 empty) with a graph on its 5 columns: the edge (0, 3) twice and reversed once,
    node 2 isolated -- it has no edge and an empty column -- and node 1 with one edge"""
    return Problem(LR.tiny(dt), [0, 0, 3, 4], [3, 3, 0, 1])


def random(dt):
    return Problem(LR.random_rows(700, 1031, 40, 7, dt), *GR.random_multigraph(1031, 5))


def tile(dt, pack):
    """one coordinate past one trial tile of the column pass"""
    n = 256 * LR.TRIAL_U * pack + 1
    return Problem(LR.random_rows(200, n, 12, 9, dt), *GR.ring_chords(n))


def long_columns(dt):
    """linear_ref.long_columns (n = 37, R = 9000) with the star whose hub is column 0, the dense one: the hub has both the
    longest edge list and chunk partials"""
    return Problem(LR.long_columns(dt), *GR.star(37, 0))
