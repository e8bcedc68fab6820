"""Mesh objectives (lbfgspp_amd.MeshObjective, csrc/mesh_kernels.cuh): the bodies the tests compile and their plain numpy
restatements, one numpy operation per source operation, in the objective's dtype.  No GPU, no library.

N nodes with D unknowns each, x node-major (x[v*D + d]); E elements of K nodes each, elems of shape (E, K).  An element
restatement returns (tg, v): tg[e, k, d] the partial derivative of element e with respect to unknown d of its slot k and v[e]
its value; a node restatement returns (g, v) with g of shape (N, D).  mesh_grad puts the gradient together by the rule of
include/lbfgsx.h: grad[v*D + d] = the node term's g[d] if there is one, then the tg[e, slot, d] of the elements that contain v
in ascending e, started from the first contribution; +0 for a node without any.  The bodies use + - * only and loop over K
and D, so one text serves every (K, D)."""
import itertools

import numpy as np

TRIAL_U = {1: 2, 2: 1, 3: 1}  # mesh_kernels.cuh: MeshTrialU<D>, the tile depth of the two trial kernels

# the statement tests' element body: another weight on every slot and every unknown, p0 per element, p1 at every node of the
# element, c0, c1 and e in the value
#   q = p0[e] sum_kd ((kD + d + 1) p1[v[k]]) x[kD + d] + (e c0 + c1),  value q^2 / 2
ASYM_ELEM = """T s = T(0);
for (int k = 0; k < K; k++)
    for (int d = 0; d < D; d++)
        s = s + (T(k * D + d + 1) * p1[v[k]]) * x[k * D + d];
const T q = p0[e] * s + (T(e) * c[0] + c[1]);
const T pq = p0[e] * q;
for (int k = 0; k < K; k++)
    for (int d = 0; d < D; d++)
        g[k * D + d] = (T(k * D + d + 1) * p1[v[k]]) * pq;
return T(0.5) * (q * q);"""
# the node body: sum_d (c2 (d + 1)) / 2 (x[d] - p2[iD + d])^2
NODE = """T s = T(0);
for (int d = 0; d < D; d++)
{
    const T r = x[d] - p2[i * D + d];
    const T k = (c[2] * T(d + 1)) * r;
    g[d] = k;
    s = s + T(0.5) * (k * r);
}
return s;"""
SCALARS = (0.003, -0.7, 0.6)  # c0, c1, c2: none is a float or a double

# a K = 3 chain body (it reads i, the term's start); as the element body of the strip, where e = t, it follows ALIAS_I
TRIPLE = """const T u = x[2] - x[0] * x[1];
const T pu = p0[i] * u;
g[2] = T(2) * pu;
g[0] = T(-2) * (pu * x[1]);
g[1] = T(-2) * (pu * x[0]);
return pu * u;"""
ALIAS_I = "const int64_t i = e;\n"
# what a graph edge body follows as a K = 2, D = 1 element body: its i and j are the element's two nodes
ALIAS_IJ = "const int64_t i = v[0], j = v[1];\n"

# the solver tests' instance (tests/cpp/mesh_probe.cpp), K = 3, D = 2: the squared deviations of the three squared edge
# lengths from p0[e], p1[e], p2[e], the squared deviation of the doubled signed area from c1 with weight c0, and a node term
# that ties each node to its rest position p3 with stiffness c2
TRIANGLE = """const T ax = x[2] - x[0], ay = x[3] - x[1];
const T bx = x[4] - x[2], by = x[5] - x[3];
const T cx = x[0] - x[4], cy = x[1] - x[5];
const T ra = (ax * ax + ay * ay) - p0[e];
const T rb = (bx * bx + by * by) - p1[e];
const T rc = (cx * cx + cy * cy) - p2[e];
const T ar = (ax * by - ay * bx) - c[1];
const T wa = c[0] * ar;
g[0] = (rc * cx - ra * ax) - wa * by;
g[1] = (rc * cy - ra * ay) + wa * bx;
g[2] = (ra * ax - rb * bx) - wa * cy;
g[3] = (ra * ay - rb * by) + wa * cx;
g[4] = (rb * bx - rc * cx) - wa * ay;
g[5] = (rb * by - rc * cy) + wa * ax;
return T(0.25) * ((ra * ra + rb * rb) + rc * rc) + T(0.5) * (wa * ar);"""
TIE_NODE = """T s = T(0);
for (int d = 0; d < D; d++)
{
    const T r = x[d] - p3[i * D + d];
    const T k = c[2] * r;
    g[d] = k;
    s = s + T(0.5) * (k * r);
}
return s;"""
# the convex instance: p0[e]/2 |x_a - x_b|^2 over all node pairs of an element, and 1/2 |x_v - p1[v]|^2 per node
PAIRS_ELEM = """for (int k = 0; k < K * D; k++)
    g[k] = T(0);
T s = T(0);
for (int a = 0; a < K; a++)
    for (int b = a + 1; b < K; b++)
        for (int d = 0; d < D; d++)
        {
            const T u = x[a * D + d] - x[b * D + d];
            const T w = p0[e] * u;
            g[a * D + d] = g[a * D + d] + w;
            g[b * D + d] = g[b * D + d] - w;
            s = s + T(0.5) * (w * u);
        }
return s;"""
FIDELITY_NODE = """T s = T(0);
for (int d = 0; d < D; d++)
{
    const T r = x[d] - p1[i * D + d];
    g[d] = r;
    s = s + T(0.5) * (r * r);
}
return s;"""
# the measurement's K = 4, D = 3 body: 1/2 (signed volume x 6 - p0[e])^2
VOLUME = """const T ax = x[3] - x[0], ay = x[4] - x[1], az = x[5] - x[2];
const T bx = x[6] - x[0], by = x[7] - x[1], bz = x[8] - x[2];
const T cx = x[9] - x[0], cy = x[10] - x[1], cz = x[11] - x[2];
const T nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
const T mx = cy * az - cz * ay, my = cz * ax - cx * az, mz = cx * ay - cy * ax;
const T lx = ay * bz - az * by, ly = az * bx - ax * bz, lz = ax * by - ay * bx;
const T r = ((ax * nx + ay * ny) + az * nz) - p0[e];
g[3] = r * nx; g[4] = r * ny; g[5] = r * nz;
g[6] = r * mx; g[7] = r * my; g[8] = r * mz;
g[9] = r * lx; g[10] = r * ly; g[11] = r * lz;
g[0] = T(0) - ((g[3] + g[6]) + g[9]);
g[1] = T(0) - ((g[4] + g[7]) + g[10]);
g[2] = T(0) - ((g[5] + g[8]) + g[11]);
return T(0.5) * (r * r);"""
# every body a test compiles for all nine (K, D): (name, element body, node body)
GENERIC_BODIES = (("asym", ASYM_ELEM, NODE), ("asym-no-node", ASYM_ELEM, None), ("pairs", PAIRS_ELEM, FIDELITY_NODE))


# ---------------------------------------------------------------- the restatements
def _xe(x, elems, D):
    """x at the nodes of every element: shape (E, K, D)"""
    return x.reshape(-1, D)[np.asarray(elems, np.int64)]


def asym_elem_terms(x, elems, D, p0, p1, scalars=SCALARS):
    dt = x.dtype.type
    elems = np.asarray(elems, np.int64)
    E, K = elems.shape
    xe = _xe(x, elems, D)
    s = np.zeros(E, x.dtype)
    for k in range(K):
        for d in range(D):
            s = s + (dt(k * D + d + 1) * p1[elems[:, k]]) * xe[:, k, d]
    e = np.arange(E).astype(x.dtype)
    q = p0 * s + (e * dt(scalars[0]) + dt(scalars[1]))
    pq = p0 * q
    tg = np.empty((E, K, D), x.dtype)
    for k in range(K):
        for d in range(D):
            tg[:, k, d] = (dt(k * D + d + 1) * p1[elems[:, k]]) * pq
    return tg, dt(0.5) * (q * q)


def _node_quadratic(x, D, p, k_of):
    """sum over d of 1/2 k r with r = x[d] - p[i*D + d], k = k_of(r, d): the shape of NODE, TIE_NODE and FIDELITY_NODE"""
    dt = x.dtype.type
    xv, pv = x.reshape(-1, D), p.reshape(-1, D)
    g = np.empty_like(xv)
    s = np.zeros(xv.shape[0], x.dtype)
    for d in range(D):
        r = xv[:, d] - pv[:, d]
        k = k_of(r, d)
        g[:, d] = k
        s = s + dt(0.5) * (k * r)
    return g, s


def node_terms(x, D, p2, scalars=SCALARS):
    dt = x.dtype.type
    return _node_quadratic(x, D, p2, lambda r, d: (dt(scalars[2]) * dt(d + 1)) * r)


def tie_terms(x, D, rest, c2):
    return _node_quadratic(x, D, rest, lambda r, d: x.dtype.type(c2) * r)


def fidelity_terms(x, D, b):
    return _node_quadratic(x, D, b, lambda r, d: r)


def triple_terms(x, elems, p0):
    """TRIPLE as the element body of the strip (D = 1): p0 is read at i = e"""
    dt = x.dtype.type
    xe = _xe(x, elems, 1)[:, :, 0]
    x0, x1, x2 = xe[:, 0], xe[:, 1], xe[:, 2]
    u = x2 - x0 * x1
    pu = p0[:xe.shape[0]] * u
    tg = np.stack([dt(-2) * (pu * x1), dt(-2) * (pu * x0), dt(2) * pu], 1)[:, :, None]
    return tg, pu * u


def triangle_terms(x, elems, l0, l1, l2, c0, c1):
    dt = x.dtype.type
    xe = _xe(x, elems, 2).reshape(-1, 6)
    X = [xe[:, k] for k in range(6)]
    ax, ay = X[2] - X[0], X[3] - X[1]
    bx, by = X[4] - X[2], X[5] - X[3]
    cx, cy = X[0] - X[4], X[1] - X[5]
    ra = (ax * ax + ay * ay) - l0
    rb = (bx * bx + by * by) - l1
    rc = (cx * cx + cy * cy) - l2
    ar = (ax * by - ay * bx) - dt(c1)
    wa = dt(c0) * ar
    g = [(rc * cx - ra * ax) - wa * by, (rc * cy - ra * ay) + wa * bx, (ra * ax - rb * bx) - wa * cy,
         (ra * ay - rb * by) + wa * cx, (rb * bx - rc * cx) - wa * ay, (rb * by - rc * cy) + wa * ax]
    return np.stack(g, 1).reshape(-1, 3, 2), dt(0.25) * ((ra * ra + rb * rb) + rc * rc) + dt(0.5) * (wa * ar)


def pairs_terms(x, elems, D, w):
    dt = x.dtype.type
    xe = _xe(x, elems, D)
    E, K = xe.shape[:2]
    tg = np.zeros((E, K, D), x.dtype)
    s = np.zeros(E, x.dtype)
    for a in range(K):
        for b in range(a + 1, K):
            for d in range(D):
                u = xe[:, a, d] - xe[:, b, d]
                wu = w * u
                tg[:, a, d] = tg[:, a, d] + wu
                tg[:, b, d] = tg[:, b, d] - wu
                s = s + dt(0.5) * (wu * u)
    return tg, s


def volume_terms(x, elems, p0):
    dt = x.dtype.type
    xe = _xe(x, elems, 3).reshape(-1, 12)
    X = [xe[:, k] for k in range(12)]
    ax, ay, az = X[3] - X[0], X[4] - X[1], X[5] - X[2]
    bx, by, bz = X[6] - X[0], X[7] - X[1], X[8] - X[2]
    cx, cy, cz = X[9] - X[0], X[10] - X[1], X[11] - X[2]
    nx, ny, nz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
    mx, my, mz = cy * az - cz * ay, cz * ax - cx * az, cx * ay - cy * ax
    lx, ly, lz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    r = ((ax * nx + ay * ny) + az * nz) - p0
    g = [None] * 12
    g[3], g[4], g[5] = r * nx, r * ny, r * nz
    g[6], g[7], g[8] = r * mx, r * my, r * mz
    g[9], g[10], g[11] = r * lx, r * ly, r * lz
    g[0] = dt(0) - ((g[3] + g[6]) + g[9])
    g[1] = dt(0) - ((g[4] + g[7]) + g[10])
    g[2] = dt(0) - ((g[5] + g[8]) + g[11])
    return np.stack(g, 1).reshape(-1, 4, 3), dt(0.5) * (r * r)


# ---------------------------------------------------------------- the gradient rule and the topology
def incidence(elems, N):
    """the incidence list lbfgsx_objective_bind_mesh builds: (off uint32[N+1], words uint32[K*E, K]) -- the K*E pairs
    (node, (e << 2) | slot) in the order e ascending, slot ascending, sorted by node with a stable sort; an entry is
    (e << 2) | slot, then the element's other nodes in ascending slot order"""
    elems = np.asarray(elems, np.int64)
    E, K = elems.shape
    keys = elems.reshape(-1)
    slot = np.tile(np.arange(K, dtype=np.int64), E)
    e = np.repeat(np.arange(E, dtype=np.int64), K)
    order = np.argsort(keys, kind="stable")
    off = np.searchsorted(keys[order], np.arange(N + 1), side="left")
    words = np.empty((K * E, K), np.int64)
    words[:, 0] = (e << 2) | slot
    for j in range(1, K):  # the (j-1)-th other node: slot j-1 below the own slot, slot j above it
        words[:, j] = elems[e, np.where(j - 1 < slot, j - 1, j)]
    return off.astype(np.uint32), words[order].astype(np.uint32)


def mesh_grad(tg, elems, N, node_g=None):
    """a stable argsort by node, then a sequential sum per node: the node term first, no leading 0 +.  Returns grad, n = N*D"""
    E, K, D = tg.shape
    dt = tg.dtype
    off, words = incidence(elems, N)
    off = off.astype(np.int64)
    es = words[:, 0].astype(np.int64)
    contrib = tg[es >> 2, es & 3, :]  # (K*E, D) in list order
    deg = np.diff(off)
    if node_g is not None:
        g, has = node_g.reshape(N, D).astype(dt, copy=True), np.ones(N, bool)
    else:
        g, has = np.zeros((N, D), dt), np.zeros(N, bool)
    for r in range(int(deg.max()) if N else 0):
        idx = np.nonzero(deg > r)[0]
        c = contrib[off[idx] + r]
        g[idx] = np.where(has[idx, None], g[idx] + c, c)
        has[idx] = True
    assert g.dtype == dt
    return g.reshape(-1)


def mesh_grad_scalar(tg, elems, N, node_g=None):
    """the same rule as a plain triple loop over nodes, elements and slots (the proof of mesh_grad)"""
    E, K, D = tg.shape
    dt = tg.dtype.type
    g = np.zeros((N, D), tg.dtype)
    for v in range(N):
        for d in range(D):
            acc = None if node_g is None else node_g.reshape(N, D)[v, d]
            for e in range(E):
                for k in range(K):
                    if elems[e][k] == v:
                        c = tg[e, k, d]
                        acc = c if acc is None else dt(acc + c)
            g[v, d] = dt(0) if acc is None else acc
    return g.reshape(-1)


# ---------------------------------------------------------------- the mesh families, each for any K and any N >= K
def strip(K, N):
    t = np.arange(N - K + 1, dtype=np.int64)
    return t[:, None] + np.arange(K, dtype=np.int64)[None, :]


def reversed_strip(K, N):
    """elements in descending t, slots in descending node order: the order of a node's sum goes by e, not by neighbour"""
    return strip(K, N)[::-1, ::-1].copy()


def fan(K, N, hub):
    """elements around the hub: the hub's slot is e mod K, the other nodes are consecutive runs of K - 1 of the remaining
    nodes (the last run reaches back when they do not divide)"""
    others = np.array([k for k in range(N) if k != hub], np.int64)
    starts = list(range(0, others.size - (K - 1) + 1, K - 1))
    if starts[-1] + (K - 1) < others.size:
        starts.append(others.size - (K - 1))
    rows = []
    for e, s in enumerate(starts):
        run = list(others[s:s + K - 1])
        run.insert(e % K, hub)
        rows.append(run)
    return np.array(rows, np.int64)


def random_mesh(K, N, seed):
    """3N elements among about nine tenths of the nodes (the rest stay isolated), with a duplicate element and a slot-permuted
    duplicate for certain, then two elements that contain both node 0 and node N-1.  For N < K + 2 every node is live"""
    rng = np.random.default_rng(seed)
    live = np.nonzero(rng.random(N) >= 0.1)[0] if N >= K + 2 else np.arange(N)
    if live.size < K:
        live = np.arange(N)
    E = 3 * N
    el = rng.choice(live, (E, K))
    while True:  # pairwise distinct nodes within an element
        s = np.sort(el, 1)
        bad = (s[:, 1:] == s[:, :-1]).any(1)
        if not bad.any():
            break
        el[bad] = rng.choice(live, (int(bad.sum()), K))
    k = E // 2
    el[k + 1] = el[k]
    el[k + 2] = np.roll(el[k], 1)
    mid = np.arange(1, K - 1, dtype=np.int64)  # K - 2 nodes that are neither 0 nor N - 1 (N >= K)
    ends = np.array([np.concatenate([[0, N - 1], mid]), np.concatenate([[N - 1], mid[::-1], [0]])], np.int64)
    return np.concatenate([el, ends]).astype(np.int64)


def lattice(K, shape):
    """the structured triangulation (K = 3, shape = (ny, nx): two counter-clockwise triangles per cell, node r*nx + c at
    (c, r)) or tetrahedralisation (K = 4, shape = (nz, ny, nx): six positively oriented tetrahedra per cube around its main
    diagonal, node (s*ny + r)*nx + c at (c, r, s)) of a lattice.  Returns (elems, rest positions of shape (N, D))"""
    if K == 3:
        ny, nx = shape
        r, c = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        i = (r * nx + c).reshape(-1)
        el = np.stack([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)], 1).reshape(-1, 3)
        rr, cc = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        return el.astype(np.int64), np.stack([cc, rr], -1).reshape(-1, 2).astype(np.float64)
    assert K == 4
    nz, ny, nx = shape
    s, r, c = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    i = ((s * ny + r) * nx + c).reshape(-1)
    step = (1, nx, nx * ny)
    tets = []
    for perm in itertools.permutations(range(3)):
        a, b, c3 = (step[p] for p in perm)
        even = perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1))
        cols = [i, i + a, i + a + b, i + a + b + c3] if even else [i, i + a + b, i + a, i + a + b + c3]
        tets.append(np.stack(cols, 1))
    el = np.stack(tets, 1).reshape(-1, 4)
    ss, rr, cc = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return el.astype(np.int64), np.stack([cc, rr, ss], -1).reshape(-1, 3).astype(np.float64)
