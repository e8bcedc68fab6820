"""Graph objectives (lbfgspp_amd.GraphObjective, csrc/graph_kernels.cuh): the bodies the tests compile and their plain numpy
restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

x has n coordinates, the nodes; the E edges are (ei[e], ej[e]).  An edge restatement returns (tg, v): tg[s][e] the partial
derivative of edge e with respect to its end s (0: ei[e], 1: ej[e]) and v[e] its value; a node restatement returns (g, v) per
node.  graph_grad puts the gradient together by the rule of include/lbfgsx.h: grad[v] = the node term's derivative if there
is one, then the tg[side][e] of the edges incident to v in ascending e, started from the first contribution; +0 for a node
without any.  The bodies use + - * only."""
import numpy as np

# the statement tests' edge body: another weight on each slot and each partial, p0 per edge, p1 per node at both ends, c0, c1
# and e in the value
#   q = (p0[e] p1[i]) x0 + 2 (p1[j] x1) + (e c0 + c1),  value q^2 / 2
ASYM_EDGE = """const T we = p0[e], wi = p1[i], wj = p1[j];
const T a = we * wi;
const T s = a * x[0] + T(2) * (wj * x[1]);
const T q = s + (T(e) * c[0] + c[1]);
g[0] = a * q;
g[1] = T(2) * (wj * q);
return T(0.5) * (q * q);"""
# the node body: c2/2 (x - p1[i])^2
NODE = """const T r = x[0] - p1[i];
const T k = c[2] * r;
g[0] = k;
return T(0.5) * (k * r);"""
SCALARS = (0.003, -0.7, 0.6)  # c0, c1, c2: none is a float or a double

# a pair term that is valid as the edge body of the path graph (e = i = t, j = t+1) and as a K = 2 chain (i = t)
PAIR = """const T u = x[1] - x[0] * x[0];
const T pu = p0[i] * u;
g[1] = T(2) * pu;
g[0] = T(-4) * (pu * x[0]);
return pu * u;"""

# the solver tests' instance (tests/cpp/graph_probe.cpp): weighted springs and a double well
SPRING_EDGE = """const T d = x[0] - x[1];
const T w = p0[e] * d;
g[0] = w;
g[1] = T(0) - w;
return T(0.5) * (w * d);"""
WELL_NODE = """const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = (T(4) * k) * (u * x[0]);
return k * (u * u);"""
# the convex instance: springs and c0-free 1/2 (x - p1[i])^2
FIDELITY_NODE = """const T r = x[0] - p1[i];
g[0] = r;
return T(0.5) * (r * r);"""


# ---------------------------------------------------------------- the restatements
def asym_edge_terms(x, ei, ej, p0, p1, scalars=SCALARS):
    dt = x.dtype.type
    x0, x1 = x[ei], x[ej]
    we, wi, wj = p0, p1[ei], p1[ej]
    c0, c1 = dt(scalars[0]), dt(scalars[1])
    e = np.arange(ei.size).astype(x.dtype)
    a = we * wi
    s = a * x0 + dt(2) * (wj * x1)
    q = s + (e * c0 + c1)
    return [a * q, dt(2) * (wj * q)], dt(0.5) * (q * q)


def node_terms(x, p1, scalars=SCALARS):
    dt = x.dtype.type
    r = x - p1
    k = dt(scalars[2]) * r
    return k, dt(0.5) * (k * r)


def pair_terms(x, ei, ej, p0):
    """PAIR as an edge body: p0 is read at i = ei[e]"""
    dt = x.dtype.type
    x0, x1 = x[ei], x[ej]
    u = x1 - x0 * x0
    pu = p0[ei] * u
    return [dt(-4) * (pu * x0), dt(2) * pu], pu * u


def spring_terms(x, ei, ej, w):
    dt = x.dtype.type
    d = x[ei] - x[ej]
    wd = w * d
    return [wd, dt(0) - wd], dt(0.5) * (wd * d)


def well_terms(x, c0):
    dt = x.dtype.type
    u = x * x - dt(1)
    k = dt(c0) * dt(0.25)
    return (dt(4) * k) * (u * x), k * (u * u)


def fidelity_terms(x, b):
    dt = x.dtype.type
    r = x - b
    return r, dt(0.5) * (r * r)


# ---------------------------------------------------------------- the gradient rule and the topology
def incidence(ei, ej, n):
    """the incidence list lbfgsx_objective_bind_graph builds: (off uint32[n+1], other int32[2E], edge_side uint32[2E]) -- the 2E
    (node, (e << 1) | side) pairs in the order e = 0 side 0, e = 0 side 1, e = 1 side 0, .. sorted by node with a stable sort"""
    ei, ej = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
    E = ei.size
    keys = np.stack([ei, ej], 1).reshape(-1)
    es = (np.repeat(np.arange(E, dtype=np.int64), 2) << 1) | np.tile(np.array([0, 1], np.int64), E)
    other = np.stack([ej, ei], 1).reshape(-1)
    order = np.argsort(keys, kind="stable")
    off = np.searchsorted(keys[order], np.arange(n + 1), side="left")
    return off.astype(np.uint32), other[order].astype(np.int32), es[order].astype(np.uint32)


def graph_grad(tg, ei, ej, n, node_g=None):
    """a stable argsort by node, then a sequential sum per node: the node term first, no leading 0 +"""
    dt = tg[0].dtype
    off, _, es = incidence(ei, ej, n)
    off = off.astype(np.int64)
    contrib = np.stack([tg[0], tg[1]], 1).reshape(-1)[es.astype(np.int64)]  # position 2e + side is es itself
    deg = np.diff(off)
    if node_g is not None:
        g, has = node_g.astype(dt, copy=True), np.ones(n, bool)
    else:
        g, has = np.zeros(n, dt), np.zeros(n, bool)
    for r in range(int(deg.max()) if n else 0):
        idx = np.nonzero(deg > r)[0]
        c = contrib[off[idx] + r]
        g[idx] = np.where(has[idx], g[idx] + c, c)
        has[idx] = True
    assert g.dtype == dt
    return g


def graph_grad_scalar(tg, ei, ej, n, node_g=None):
    """the same rule as a plain double loop over nodes and edges (the proof of graph_grad)"""
    dt = tg[0].dtype.type
    g = np.zeros(n, tg[0].dtype)
    for v in range(n):
        acc = None if node_g is None else node_g[v]
        for e in range(len(ei)):
            for side, end in ((0, ei[e]), (1, ej[e])):
                if end == v:
                    c = tg[side][e]
                    acc = c if acc is None else dt(acc + c)
        g[v] = dt(0) if acc is None else acc
    return g


# ---------------------------------------------------------------- the graph families
def path(n):
    t = np.arange(n - 1, dtype=np.int64)
    return t, t + 1


def reversed_path(n):
    """edges (t+1, t), listed in descending t: the order of a node's contributions goes by e, not by neighbour"""
    t = np.arange(n - 2, -1, -1, dtype=np.int64)
    return t + 1, t


def star(n, hub):
    """every other node joined to the hub, the hub alternately the edge's end 0 and end 1"""
    v = np.array([k for k in range(n) if k != hub], np.int64)
    flip = (np.arange(v.size) & 1).astype(bool)
    return np.where(flip, hub, v), np.where(flip, v, hub)


def random_multigraph(n, seed):
    """E = 3n edges among about nine tenths of the nodes (the rest stay isolated), duplicates included, then (0, n-1) and
    (n-1, 0).  For n < 4 every node is live"""
    rng = np.random.default_rng(seed)
    live = np.nonzero(rng.random(n) >= 0.1)[0] if n >= 4 else np.arange(n)
    if live.size < 2:
        live = np.arange(n)
    E = 3 * n
    i = rng.choice(live, E)
    j = rng.choice(live, E)
    same = i == j
    while same.any():  # no self-loops
        j[same] = rng.choice(live, int(same.sum()))
        same = i == j
    k = E // 2
    i[k + 1], j[k + 1] = i[k], j[k]  # a duplicate for certain
    return np.concatenate([i, [0, n - 1]]).astype(np.int64), np.concatenate([j, [n - 1, 0]]).astype(np.int64)


def ring_chords(n):
    """the solver tests' graph (tests/cpp/graph_probe.cpp): for t = 0 .. n-1 the edge (t, (t+1) mod n), then, when t mod 3 = 0
    and u = (7t + 3) mod n differs from t, the chord (u, t)"""
    ei, ej = [], []
    for t in range(n):
        ei.append(t)
        ej.append((t + 1) % n)
        u = (7 * t + 3) % n
        if t % 3 == 0 and u != t:
            ei.append(u)
            ej.append(t)
    return np.array(ei, np.int64), np.array(ej, np.int64)


def ring_weights(E, dtype=np.float64):
    return (1.0 + 0.25 * (np.arange(E) % 5)).astype(dtype)
