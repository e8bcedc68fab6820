"""Exact reference of the L-BFGS two-loop recursion d = a H v (BFGSMat::apply_Hv, BFGSMat.h:276-302) and of the post
statements that feed it, for the statement-level tests of the unbounded path.  Plain numpy and Python: no GPU, no oracle
library.  tests/test_twoloop_ref_cpu.py proves what is here, tests/test_twoloop_statements_gpu.py uses it.

The contract restated:
  * element-wise statements are IEEE in the scalar type T, one rounding per source operation, no contraction: numpy in the
    same dtype, one numpy operation per operation of the source;
  * every dot is the exact sum (statement_ref.exact_dot) rounded as the accumulators round it (bounded_sums_ref.stored: to
    double, and for f32 then to float);
  * the coefficients are plain T divisions.
So d, the 2c+1 dots and v.d are determined bit for bit by the inputs -- as long as no exact sum lies so close to a rounding
boundary that the accumulator's own error (bounded_sums_ref.dd_bound / sum_bound) could tip it.  Every dot carries that flag;
the tests assert that no dot of any case has it, and the seeds of the cases below were chosen on the CPU so that none does.
"""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

import bounded_sums_ref as B
import statement_ref as R

F64, F32 = np.float64, np.float32

Dot = namedtuple("Dot", "value exact bound ambiguous")        # value: the T-rounded sum as a T scalar
TwoLoop = namedtuple("TwoLoop", "d dots dg ambiguous order ys theta alpha")
Post = namedtuple("Post", "s y sums accepted ys theta S Y ptr ncorr two_loop")


# ---------------------------------------------------------------- dots
def _sum_abs_upper(a, b):
    """an upper estimate of sum |a_i b_i| (numpy's blocked sum in double errs by far less than 2^-20 relative)"""
    sabs = float(np.dot(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64)))
    return Fraction(sabs) * (1 + Fraction(1, 1 << 20))


def rdot(a, b, dtype):
    """sum a_i b_i as the kernels deliver it: the exact sum rounded to double and (f32) then to float, with the accumulator's
    worst-case error (dd_bound for f64, sum_bound for f32) and whether the exact sum lies within it of a rounding boundary"""
    dt = np.dtype(dtype).type
    a, b = np.ascontiguousarray(a, dt), np.ascontiguousarray(b, dt)
    ex = R.exact_dot(a, b)
    sabs = _sum_abs_upper(a, b)
    if dt == np.float64 or _cannot_be_exact(a, b, sabs):
        bound = B.dd_bound(a.size, sabs)
    else:
        bound = B.sum_bound(a.size, sabs, a, b)
    return Dot(dt(B.stored(ex, dt)), ex, bound, B.is_ambiguous(ex, bound, dt))


def _cannot_be_exact(a, b, sabs):
    """sum_bound returns 0 only where 2 n sum|ab| < 2^106 2^(la + lb) with 2^la, 2^lb the lowest set bits over the columns, and
    2^la is at most the smallest non-zero |a_i|: where the test fails with those in place of the low bits, sum_bound is dd_bound
    and its scan of the mantissas (the dearer half of an f32 reference at 10^7 elements) is skipped"""
    an, bn = np.abs(a[a != 0]), np.abs(b[b != 0])
    if an.size == 0 or bn.size == 0:
        return False
    return 2 * a.size * sabs >= (1 << 106) * Fraction(float(an.min())) * Fraction(float(bn.min()))


# ---------------------------------------------------------------- the ring (BFGSMat.h:42-48, 81-97)
def ring_order(ptr, m, c):
    """storage slots newest -> oldest (BFGSMat.h:284-287)"""
    out, j = [], ptr % m
    for _ in range(c):
        j = (j + m - 1) % m
        out.append(j)
    return out


def ring_add(slots, ptr, m, pair):
    """BFGSMat::add_correction on a list of (s, y) by storage slot; returns the new ptr"""
    loc = ptr % m
    if loc < len(slots):
        slots[loc] = pair
    else:
        assert loc == len(slots)
        slots.append(pair)
    return loc + 1


def ring_fill(pairs, m):
    """the history after feeding `pairs` in order to an empty ring of length m: (S, Y, ptr) with S, Y of shape [c, n] in
    storage-slot order -- what lbfgsx_bfgs_download_history returns"""
    slots, ptr = [], m
    for p in pairs:
        ptr = ring_add(slots, ptr, m, p)
    if not slots:
        return None, None, ptr
    return np.stack([p[0] for p in slots]), np.stack([p[1] for p in slots]), ptr


def pair_scalars(s, y, dtype):
    """(ys, theta, Dot s.y, Dot y.y) of one pair: ys = T(s.y), theta = T(y.y) / T(s.y) (BFGSMat.h:89-92) from exact dots, as
    lbfgsx_bfgs_stage_correction_host and k_post form them"""
    sy, yy = rdot(s, y, dtype), rdot(y, y, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return sy.value, yy.value / sy.value, sy, yy


# ---------------------------------------------------------------- BFGSMat.h:276-302
def two_loop(S, Y, ptr, m, v, a, g=None, dtype=F64, scalars=None):
    """d = a H v.  S, Y: [c, n] in storage-slot order (None or empty: no pair), ptr as in BFGSMat.h:42-48; g: the vector
    the last dot is taken against (None: v itself).  scalars: {slot: (ys, theta)} where the caller has them already.
    Returns d, the 2c+1 dots (c of the first loop, c of the second, then g.d) as Dot records, g.d as a float, whether any
    dot is ambiguous, and the column order, ys, theta (of the newest pair) and alpha the recursion used."""
    dt = np.dtype(dtype).type
    c = 0 if S is None else len(S)
    order = ring_order(ptr, m, c)
    ys, th = {}, {}
    for j in order:
        if scalars is not None and j in scalars:
            ys[j], th[j] = scalars[j]
        else:
            ys[j], th[j] = pair_scalars(S[j], Y[j], dt)[:2]
    v = np.ascontiguousarray(v, dt)
    dots = []
    q = dt(a) * v                                        # res = a * v                     (:283)
    alpha = {}
    for j in order:                                      # newest -> oldest                (:284-290)
        dots.append(rdot(S[j], q, dt))
        alpha[j] = dots[-1].value / ys[j]                # alpha_j = s_j.res / ys_j        (:288)
        t = alpha[j] * Y[j]
        q = q - t                                        # res -= alpha_j y_j              (:289)
    theta = th[order[0]] if c else dt(1)
    if c:
        q = q / theta                                    # res /= theta                    (:293)
    for j in reversed(order):                            # oldest -> newest                (:296-301)
        dots.append(rdot(Y[j], q, dt))
        beta = dots[-1].value / ys[j]                    # beta = y_j.res / ys_j           (:298)
        t = (alpha[j] - beta) * S[j]
        q = q + t                                        # res += (alpha_j - beta) s_j     (:299)
    dots.append(rdot(v if g is None else np.ascontiguousarray(g, dt), q, dt))
    assert len(dots) == 2 * c + 1 and q.dtype == dt
    return TwoLoop(q, dots, float(dots[-1].value), any(d.ambiguous for d in dots), order, ys, theta, alpha)


def post_then_two_loop(x, xp, g, gp, S, Y, ptr, m, a, eps=None, dtype=F64):
    """The statements after a line search and the recursion that follows (LBFGS.h:130,137,159-165), as the fused launch
    runs them: s = x - xp, y = g - gp in T; the sums g.g, x.x, s.y, y.y; the pair is usable iff T(s.y) > eps * T(y.y) with
    eps the machine epsilon of T (None), the product taken in T; ys and theta of the pair; then d = a H g on the history with
    the pair added (accepted) or on the history as it was (rejected)."""
    dt = np.dtype(dtype).type
    s, y = x - xp, g - gp
    assert s.dtype == dt and y.dtype == dt
    sums = [rdot(g, g, dt), rdot(x, x, dt), rdot(s, y, dt), rdot(y, y, dt)]
    sy, yy = sums[2].value, sums[3].value
    e = dt(np.finfo(dt).eps if eps is None else eps)
    accepted = bool(sy > e * yy)
    with np.errstate(divide="ignore", invalid="ignore"):
        ys, theta = sy, yy / sy
    c = 0 if S is None else len(S)
    slots = [(S[j], Y[j]) for j in range(c)]
    scal = None
    if accepted:
        loc = ptr % m
        ptr = ring_add(slots, ptr, m, (s, y))
        scal = {loc: (ys, theta)}
    S2 = np.stack([p[0] for p in slots]) if slots else None
    Y2 = np.stack([p[1] for p in slots]) if slots else None
    tl = two_loop(S2, Y2, ptr, m, g, a, None, dt, scalars=scal)
    return Post(s, y, sums, accepted, ys, theta, S2, Y2, ptr, len(slots), tl)


# ---------------------------------------------------------------- inputs
# persist_grid * 256 of an MI355X (2 blocks on each of 256 CUs): global threads of the persistent launch.  The sizes that
# straddle its slot classes are built from it; the GPU file asserts that the device it runs on has this value.
GTH = 512 * 256
NR, NL = 30, 15        # kPersistNR, kPersistNL: 16-byte slots of q per thread in registers / in LDS
TILE = 1024            # 16-byte vectors per tile of the step kernels and of the persistent launch's streamed part


def width(dtype):
    return 16 // np.dtype(dtype).itemsize


# family: "hist" (y = s (1 + u) + noise, the existing tests' history), "mag" (columns of magnitudes 2^-30 .. 2^30),
#         "orth" (v orthogonal to the newest s up to a 2^-16 share of sum |s_i v_i|), "aplus" ("hist" with a = +1),
#         "other" ("hist" with a gradient g that is not v: what the last dot is taken against),
#         "blocks" (the sizes from a quarter of a million elements on, see build_case)
Case = namedtuple("Case", "family n m npairs dtype seed")
Built = namedtuple("Built", "case pairs v g a")


def case_id(cs):
    return "%s-n%d-m%d-p%d-%s-s%d" % (cs.family, cs.n, cs.m, cs.npairs, np.dtype(cs.dtype).name, cs.seed)


def _block_pair(rng, n, i, k, dt, sign=1.0):
    """Pair i of k of the "blocks" inputs.
    dd_bound grows with n^2 sum|ab|: at 10^7 elements it reaches the double ulp of a sum whose terms cancel as those of
    independent normal columns do (sum|ab| ~ sqrt(n) |sum ab|), and every dot would count as ambiguous.  Here every dot of the
    recursion has terms of (nearly) one sign: pair i is positive and of order one on the i-th share of the rows and
    2^-10-sized noise elsewhere, y takes two very different values independently of s (so that y.q keeps a wide gap after s.q
    has been projected out), and v is positive.  Measured sum|ab| / |sum ab| of the 2c+1 dots: 1.0 .. 1.3."""
    edges = np.linspace(0, n, k + 1).astype(np.int64)
    row = np.arange(n)
    inside = (row >= edges[i]) & (row < edges[i + 1])
    s = np.where(inside, 0.5 + rng.random(n), 2.0 ** -10 * rng.standard_normal(n))
    y = np.where(inside, sign * np.where(rng.random(n) < 0.5, 0.25, 2.0) * (1.0 + 0.1 * rng.random(n)),
                 2.0 ** -10 * rng.standard_normal(n))
    return s.astype(dt), y.astype(dt)


def build_case(cs):
    dt = np.dtype(cs.dtype).type
    n, k = cs.n, cs.npairs
    rng = np.random.default_rng([cs.seed, n, cs.m, k, {"hist": 1, "mag": 2, "orth": 3, "aplus": 4, "other": 5, "blocks": 6}[cs.family]])
    pairs = []
    if cs.family == "blocks":
        pairs = [_block_pair(rng, n, i, k, dt) for i in range(k)]
        return Built(cs, pairs, (0.5 + rng.random(n)).astype(dt), None, -1.0)
    for i in range(k):
        s = rng.standard_normal(n)
        y = s * (1.0 + rng.random(n)) + 0.05 * rng.standard_normal(n)   # s.y > 0 like a real curvature pair
        if cs.family == "mag":
            # exact scalings: pair i lives at 2^e_i (s) and 2^f_i (y), both spread over -30 .. 30, in opposite order
            e = int(round(-30 + 60 * (i / max(k - 1, 1)))) if k > 1 else 30
            s, y = np.ldexp(s, e), np.ldexp(y, -e if k > 1 else -30)
        pairs.append((s.astype(dt), y.astype(dt)))
    v = rng.standard_normal(n)
    if cs.family == "orth" and k:
        s0 = pairs[-1][0].astype(np.float64)
        v = v - (np.dot(s0, v) / np.dot(s0, s0)) * s0
        v = v + (2.0 ** -16 * np.dot(np.abs(s0), np.abs(v)) / np.dot(s0, s0)) * s0
    v = v.astype(dt)
    g = rng.standard_normal(n).astype(dt) if cs.family == "other" else None
    return Built(cs, pairs, v, g, 1.0 if cs.family == "aplus" else -1.0)


@functools.lru_cache(maxsize=None)
def built(cs):
    return build_case(cs)


@functools.lru_cache(maxsize=None)
def reference(cs):
    """(S, Y, ptr, TwoLoop) of a case: computed once, shared by every test and form that runs the case, never modified"""
    bt = built(cs)
    S, Y, ptr = ring_fill(bt.pairs, cs.m)
    return S, Y, ptr, two_loop(S, Y, ptr, cs.m, bt.v, bt.a, bt.g, cs.dtype)


def _dedupe(cases):
    seen, out = set(), []
    for cs in cases:
        if cs not in seen:
            seen.add(cs)
            out.append(cs)
    return out


def _both(f):
    return [cs for dt in (F64, F32) for cs in f(dt, width(dt))]


N_C = 1030   # the history-length cases: one tile, a tail in f64 and in f32
M_C = 5
HISTORY_PAIRS = [0, 1, 2, M_C, M_C + 3]          # c = 0, 1, 2, m, and the ring wrapped
N_FAMILY = 4099

# the step launches (LBFGSX_PERSIST=0)
STEP_EDGE = _both(lambda dt, W: [Case("hist", n, 3, 2, dt, 1) for n in
                                 sorted({1, max(W - 1, 1), W, W + 1, TILE * W - 1, TILE * W + 1})])
# three tiles, a partial tile and a tail: run twice in a row on one context, so both traversal directions
STEP_REV = _both(lambda dt, W: [Case("hist", 3 * TILE * W + 300 * W + (W - 1), 3, 2, dt, 1)])
# more than 512 tiles: the grid (capped at 512 blocks) takes its stride twice
STEP_STRIDE = _both(lambda dt, W: [Case("blocks", 513 * TILE * W + 5 * W + 1, 2, 1, dt, 1)])
HISTORY = _both(lambda dt, W: [Case("hist", N_C, M_C, p, dt, 2) for p in HISTORY_PAIRS])
FAMILIES = _both(lambda dt, W: [Case("mag", N_FAMILY, 7, 7, dt, 3), Case("mag", N_FAMILY, 4, 7, dt, 3),
                                Case("orth", N_FAMILY, 4, 3, dt, 3), Case("aplus", N_FAMILY, 4, 3, dt, 3)])
OTHER_V = _both(lambda dt, W: [Case("other", N_FAMILY, 4, 3, dt, 4), Case("other", N_C, 4, 0, dt, 4)])
STEP_M129 = _both(lambda dt, W: [Case("hist", N_C, 129, 133, dt, 5)])   # past the persistent launch's column list

# the persistent launch, under both forms of the meeting points
PERSIST_EDGE = _both(lambda dt, W: [Case("hist", n, 3, 2, dt, 1) for n in (W, 260 * W + 1)] +
                     [Case("blocks", n, 3, 2, dt, 1) for n in ((GTH - 1) * W, (GTH + 1) * W)])   # slot 0 -> slot 1
PERSIST_M128 = _both(lambda dt, W: [Case("hist", N_C, 128, 131, dt, 5)])
# c = 2: the last register slot / the first LDS slot; then past the LDS slots: a streamed part of two tiles, a partial tile
# and a scalar tail
# (the seeds: the first from 6 on at which the reference shows no ambiguous dot; about every second one does at these sizes)
LARGE_SEED = {(F64, "lo"): 7, (F64, "hi"): 6, (F64, "stream"): 6, (F32, "lo"): 6, (F32, "hi"): 8, (F32, "stream"): 9}
LARGE_SLOTS = _both(lambda dt, W: [Case("blocks", (NR * GTH - 1) * W + 1, 2, 2, dt, LARGE_SEED[dt, "lo"]),
                                   Case("blocks", (NR * GTH + 1) * W + 1, 2, 2, dt, LARGE_SEED[dt, "hi"])])
LARGE_STREAM = _both(lambda dt, W: [Case("blocks", ((NR + NL) * GTH + 2 * TILE + 37) * W + (W - 1), 2, 2, dt, LARGE_SEED[dt, "stream"])])

STEP_CASES = _dedupe(STEP_EDGE + STEP_REV + STEP_STRIDE + HISTORY + FAMILIES + OTHER_V + STEP_M129)
PERSIST_CASES = _dedupe(PERSIST_EDGE + HISTORY + FAMILIES + OTHER_V + PERSIST_M128)
LARGE_CASES = LARGE_SLOTS + LARGE_STREAM


def small_cases():
    """every case the GPU file runs apart from the large persistent ones"""
    return _dedupe(STEP_CASES + PERSIST_CASES)


# ---------------------------------------------------------------- the fused post form (lbfgsx_post_linesearch_spec)
# n, ring length, pairs before the new one, accepted, scalar type, seed
PostCase = namedtuple("PostCase", "n m npairs accept dtype seed")
PostBuilt = namedtuple("PostBuilt", "case pairs x xp g gp")


def post_case_id(cs):
    return "n%d-m%d-p%d-%s-%s-s%d" % (cs.n, cs.m, cs.npairs, "accept" if cs.accept else "reject", np.dtype(cs.dtype).name, cs.seed)


@functools.lru_cache(maxsize=None)
def post_built(cs):
    dt = np.dtype(cs.dtype).type
    n = cs.n
    rng = np.random.default_rng([cs.seed, n, cs.m, cs.npairs, 11])
    pairs = []
    if n >= 1 << 18:
        # the "blocks" inputs: the stored pairs and the new one each on a share of the rows, the points and gradients positive
        k = cs.npairs + 1
        pairs = [_block_pair(rng, n, i, k, dt) for i in range(cs.npairs)]
        s_new, y_new = _block_pair(rng, n, cs.npairs, k, dt, 1.0 if cs.accept else -1.0)
        xp, g = (1.0 + rng.random(n)).astype(dt), (0.5 + rng.random(n)).astype(dt)
        return PostBuilt(cs, pairs, xp + s_new, xp, g, g - y_new)
    for _ in range(cs.npairs):
        s = rng.standard_normal(n)
        pairs.append((s.astype(dt), (s * (1.0 + rng.random(n)) + 0.05 * rng.standard_normal(n)).astype(dt)))
    xp, gp = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    s_new = rng.standard_normal(n)
    y_new = (1.5 if cs.accept else -1.5) * s_new + 0.05 * rng.standard_normal(n)
    return PostBuilt(cs, pairs, (xp + s_new.astype(dt)).astype(dt), xp, (gp + y_new.astype(dt)).astype(dt), gp)


@functools.lru_cache(maxsize=None)
def post_reference(cs):
    """(S, Y, ptr before the pair, Post)"""
    bt = post_built(cs)
    S, Y, ptr = ring_fill(bt.pairs, cs.m)
    return S, Y, ptr, post_then_two_loop(bt.x, bt.xp, bt.g, bt.gp, S, Y, ptr, cs.m, -1.0, None, cs.dtype)


def _post(dt, W):
    small, tail = 260 * W, TILE * W + W + (W - 1)
    out = []
    for n in (small, tail):
        for accept in (True, False):
            out += [PostCase(n, 4, 0, accept, dt, 7), PostCase(n, 4, 4, accept, dt, 7), PostCase(n, 4, 6, accept, dt, 7)]
    return out


POST_CASES = [cs for dt in (F64, F32) for cs in _post(dt, width(dt))]
POST_LARGE_SEED = {F64: 8, F32: 8}   # chosen like LARGE_SEED
POST_LARGE = [PostCase(((NR + NL) * GTH + 2 * TILE + 37) * width(dt) + (width(dt) - 1), 2, 1, True, dt, POST_LARGE_SEED[dt])
              for dt in (F64, F32)]


# ---------------------------------------------------------------- a driver's first iterations on the diagonal quadratic
Iter = namedtuple("Iter", "xp gp d dg x g post")


def quad_iterations(a, b, x0, m, steps, dtype):
    """The statements of LBFGSSolver::minimize on ObjQuad with every search accepting its first trial at the given step:
    iteration k starts at (xp, gp) with the direction d (d.gp = dg), the trial x = xp + step d is accepted, g = grad f(x), then the
    post statements and the next direction.  Returns one Iter per step; Iter.post (a Post) holds the statements after the
    trial and the direction of the next iteration."""
    dt = np.dtype(dtype).type
    x = np.ascontiguousarray(x0, dt)
    g = R.quad_ref(x, a, b)[0]
    S = Y = None
    ptr = m
    tl = two_loop(None, None, ptr, m, g, -1.0, None, dt)
    out = []
    for step in steps:
        xp, gp, d, dg = x, g, tl.d, tl.dg
        x = R.axpy_ref(xp, d, step)
        g = R.quad_ref(x, a, b)[0]
        post = post_then_two_loop(x, xp, g, gp, S, Y, ptr, m, -1.0, None, dt)
        assert post.accepted
        S, Y, ptr, tl = post.S, post.Y, post.ptr, post.two_loop
        out.append(Iter(xp, gp, d, dg, x, g, post))
    return out


# the launch from the gradient and the deferred last step: a small size, one with a partial tile and a tail, and the first size
# with a second resident slot
QUAD_M = 3
QUAD_STEPS = (2.0 ** -7, 1.0, 0.75)
QUAD_CASES = [(dt, n) for dt in (F64, F32) for n in (260 * width(dt), TILE * width(dt) + width(dt) + (width(dt) - 1),
                                                     (GTH + 1) * width(dt))]
QuadRef = namedtuple("QuadRef", "a b x0 iters")


@functools.lru_cache(maxsize=None)
def quad_reference(dtype, n):
    """f = 0.5 sum (a_i x_i - b_i)^2 with a from 1 to 10, from x0 = 0: the first len(QUAD_STEPS) iterations"""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng([9, n])
    a = 1.0 + 9.0 * (np.arange(n) / max(n - 1, 1))
    b = a * (4.0 * rng.random(n) - 2.0)
    a, b, x0 = a.astype(dt), b.astype(dt), np.zeros(n, dt)
    return QuadRef(a, b, x0, quad_iterations(a, b, x0, QUAD_M, QUAD_STEPS, dt))
